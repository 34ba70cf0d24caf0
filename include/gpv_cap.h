/* C ABI of libgpv_cap.so: device-side Bleu / CIDEr-D caption scoring for train-time evaluation (gpv-1_amd/csrc/caption_score.hip).
 *
 * A library of its own beside libgpv_hip.so (the hot path) and libgpv_eval.so (detection AP): both of those export lists are pinned.
 * Every function takes plain device pointers, returns a hipError_t as int (0 = ok), allocates nothing and keeps no global state. */
#ifndef GPV_CAP_H
#define GPV_CAP_H
#ifdef __cplusplus
extern "C" {
#endif

#define GPV_CAP_ORDERS 4         /* n-grams of 1..4 words */
#define GPV_CAP_MAX_LEN 64       /* words per caption: LH, LR and every length */
#define GPV_CAP_MAX_REFS 8       /* references per entry: R and every ref_count */
#define GPV_CAP_MAX_WORD 65535   /* word ids are 1..65535 (0 is padding): four ids make one exact 64-bit n-gram key */

/* error word bits (the word is zeroed by the call and written by the kernels; 0 = the outputs are valid) */
#define GPV_CAP_ERR_TABLE_FULL 1 /* the n-gram table had no free slot: capacity too small for the references */
#define GPV_CAP_ERR_WORD_ID 2    /* a word id inside a caption's length is < 1 or > GPV_CAP_MAX_WORD */
#define GPV_CAP_ERR_LOOKUP 4     /* a reference n-gram was not found in the table (follows from one of the above) */

/* Per-entry Bleu counts and CIDEr-D scores, the rule of gpv1_amd.evaluators.caption_scores_host.  An entry is one hypothesis and
 * ref_count[i] references; captions are int32 word ids, row-padded with 0.
 *   n-gram identity is exact: the ids of a window are packed 16 bits each into a 64-bit key (no hash decides equality);
 *   pass 1 (one workgroup per entry): every DISTINCT n-gram of the entry's references adds 1 to its document frequency in an
 *     open-addressing table in global memory (64-bit compare-and-swap on the key, integer add on the count) -- one increment per
 *     entry however many references or positions hold the n-gram; integers, so the result does not depend on arrival order;
 *   pass 2 (one workgroup per entry, windows and terms in LDS, float64 throughout, no float atomics, nothing floating leaves the
 *     workgroup): testlen, reflen (closest length, the shorter on a tie), guess[k] = max(0, testlen - k), correct[k] (clipped
 *     matches), and cider = 10 * sum_n sum_refs val[n] / 4 / ref_count with val[n] as the host rule states it, read from the two
 *     tables the caller computed once: weight[d] = log(N) - log(max(1, d)), d = 0..N, and pen[d] = e^(-d^2 / 72), d = 0..pen_len-1.
 * Every device loop is bounded by a shape or by the capacity, never by the data: lengths and counts outside their range are clamped,
 * a probe visits at most `capacity` slots, a full table sets GPV_CAP_ERR_TABLE_FULL and the call completes.
 * Shapes: N >= 0 (0: nothing is launched), 1 <= LH, LR <= GPV_CAP_MAX_LEN, 1 <= R <= GPV_CAP_MAX_REFS, pen_len >= max(LH, LR),
 * capacity a power of two >= 2 (size it to at least twice the number of reference n-gram occurrences, at most 2 * N * R * 4 * LR).
 * Workspace (contents irrelevant on entry, zeroed by the call on the stream): table_keys [capacity] 64-bit, table_df [capacity].
 * Outputs: testlen [N], reflen [N], guess [N,4], correct [N,4], cider [N], err [1]; ref_df may be NULL, else [N,R,4,LR]: the document
 * frequency of the (n+1)-gram that starts at each reference position, 0 where none starts.  An entry with ref_count 0 scores
 * cider 0 and reflen 0.  Anything outside the shapes above returns hipErrorInvalidValue before a launch. */
int gpv_cap_scores(const int* hyp /*[N,LH]*/, const int* hyp_len /*[N]*/, const int* ref /*[N,R,LR]*/, const int* ref_len /*[N,R]*/,
                   const int* ref_count /*[N]*/, int N, int LH, int R, int LR,
                   const double* weight /*[N+1]*/, const double* pen /*[pen_len]*/, int pen_len,
                   unsigned long long* table_keys /*[capacity]*/, int* table_df /*[capacity]*/, long long capacity,
                   int* testlen /*[N]*/, int* reflen /*[N]*/, int* guess /*[N,4]*/, int* correct /*[N,4]*/, double* cider /*[N]*/,
                   int* ref_df /*[N,R,4,LR] or NULL*/, int* err /*[1]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif
