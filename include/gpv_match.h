/* C ABI of libgpv_match.so: device-side Hungarian matching and DETR set criterion for box batches (gpv-1_amd/csrc/set_match.hip).
 *
 * A library of its own beside libgpv_hip.so, libgpv_eval.so and libgpv_cap.so: those three export lists are pinned.
 * Every function takes plain device pointers, returns a hipError_t as int (0 = ok), launches on `stream`, never synchronises,
 * allocates nothing and keeps no global state.  Anything outside the stated shapes returns hipErrorInvalidValue before a launch. */
#ifndef GPV_MATCH_H
#define GPV_MATCH_H
#ifdef __cplusplus
extern "C" {
#endif

#define GPV_MATCH_MAX_DIM 256     /* max(Q, Gmax): rows and columns of one assignment problem */
#define GPV_MATCH_TILE 1280       /* Q * Gmax up to which gpv_match_boxes keeps the cost of a problem in LDS and needs no cost_out */
#define GPV_MATCH_MAX_CLASSES 64  /* C + 1 of gpv_match_set_loss and gpv_match_boxes */

/* status word of a problem (0 = its indices are valid) */
#define GPV_MATCH_ERR_INVALID 1     /* a cost entry inside the problem is NaN or -inf (scipy raises "matrix contains invalid numeric entries") */
#define GPV_MATCH_ERR_INFEASIBLE 2  /* a path search found only +inf (scipy raises "cost matrix is infeasible") */
#define GPV_MATCH_ERR_DEGENERATE 4  /* a predicted or target box of the problem has x1 < x0 or y1 < y0 (the host path asserts) */

/* The linear sum assignment of P problems, the rule of gpv1_amd.criterion.lsap_host (scipy.optimize.linear_sum_assignment's
 * shortest augmenting paths, ties included).  Problem p is the Q x g_count[p] matrix cost[p, :, :g_count[p]] (row stride Gmax);
 * g_count[p] <= 0 is an empty problem.  One wave per problem, four problems per workgroup, float64 duals in LDS; every loop is
 * bounded by Q or g_count, never by the data.
 * Outputs: n_pairs[p] = min(Q, max(g_count[p], 0)) (0 when status[p] != 0), pred_idx[p, k] / tgt_idx[p, k] for k < n_pairs[p] sorted
 * by pred_idx (entries behind n_pairs[p] are -1), status[p] one of the GPV_MATCH_ERR_* bits or 0.
 * Shapes: P >= 0 (0: nothing is launched), 1 <= Q <= GPV_MATCH_MAX_DIM, 1 <= Gmax <= GPV_MATCH_MAX_DIM, g_count[p] <= Gmax,
 * Kmax >= min(Q, Gmax). */
int gpv_match_lsap(const float* cost /*[P,Q,Gmax]*/, const int* g_count /*[P]*/, int P, int Q, int Gmax, int Kmax,
                   int* pred_idx /*[P,Kmax]*/, int* tgt_idx /*[P,Kmax]*/, int* n_pairs /*[P]*/, int* status /*[P]*/, void* stream);

/* Matching cost and assignment in one launch for L layers of B images: problem (l, b) matches the Q predictions of layer l for
 * image b with the g_count[b] targets of image b.  The cost is the rule of gpv1_amd.criterion.match_cost_host, fp32, every product
 * and sum rounded on its own:  cost = (w_bbox * l1 + w_class * (-p)) + w_giou * (-giou),  p = softmax(logits)[label],
 * l1 = ((|dcx| + |dcy|) + |dw|) + |dh|, giou of the xyxy corners as generalized_box_iou orders it.
 * g_count[b] = -1: image b takes no part in localisation (n_pairs 0, status 0); g_count[b] = 0: an image without boxes (n_pairs 0).
 * cost_out [L,B,Q,Gmax] receives the cost (columns behind g_count[b] are left alone); it may be NULL when Q * Gmax <= GPV_MATCH_TILE
 * and is the required workspace beyond that.  Outputs and limits as gpv_match_lsap with P = L * B; 2 <= C1 <= GPV_MATCH_MAX_CLASSES,
 * labels outside 0..C1-1 set GPV_MATCH_ERR_INVALID. */
int gpv_match_boxes(const float* logits /*[L,B,Q,C1]*/, const float* boxes /*[L,B,Q,4] cxcywh*/, const float* tgt_boxes /*[B,Gmax,4] cxcywh*/,
                    const int* tgt_labels /*[B,Gmax]*/, const int* g_count /*[B]*/, int L, int B, int Q, int C1, int Gmax, int Kmax,
                    float w_class, float w_bbox, float w_giou, float* cost_out /*[L,B,Q,Gmax] or NULL*/,
                    int* pred_idx /*[L*B,Kmax]*/, int* tgt_idx /*[L*B,Kmax]*/, int* n_pairs /*[L*B]*/, int* status /*[L*B]*/, void* stream);

/* The DETR set criterion of the matched pairs, one workgroup per (l, b), float64 inside, fixed summation order, no float atomics,
 * nothing floating crosses a workgroup.  partial[l, b] = { sum_q w_q * ce_q, sum_q w_q, sum_pairs l1, sum_pairs (1 - giou) } with the
 * class weights 1 ... 1, eos_coef (class C1 - 1 is "no object", the target of every unmatched prediction).  The gradients are those
 * of the four sums, UNNORMALISED: dlogits of partial[..., 0], dboxes_l1 of partial[..., 2], dboxes_giou of partial[..., 3]; rows of
 * unmatched predictions are written as zeros (two arrays for the boxes because the two losses carry different weights upstream).
 * An image with g_count[b] = -1 contributes nothing: zero sums, zero gradients.  A problem whose status (as gpv_match_boxes left it,
 * degenerate boxes included) is not 0 gets NaN sums, so that it cannot pass unnoticed.
 * num_boxes [1] receives max(sum_b max(g_count[b], 0), 1) as a float64 (written by workgroup 0). */
int gpv_match_set_loss(const float* logits /*[L,B,Q,C1]*/, const float* boxes /*[L,B,Q,4]*/, const float* tgt_boxes /*[B,Gmax,4]*/,
                       const int* tgt_labels /*[B,Gmax]*/, const int* g_count /*[B]*/, const int* pred_idx /*[L*B,Kmax]*/,
                       const int* tgt_idx /*[L*B,Kmax]*/, const int* n_pairs /*[L*B]*/, int L, int B, int Q, int C1, int Gmax, int Kmax,
                       float eos_coef, double* partial /*[L,B,4]*/, float* dlogits /*[L,B,Q,C1]*/, float* dboxes_l1 /*[L,B,Q,4]*/,
                       float* dboxes_giou /*[L,B,Q,4]*/, double* num_boxes /*[1]*/, const int* status /*[L*B]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif
