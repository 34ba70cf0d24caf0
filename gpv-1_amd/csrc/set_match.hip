// Hungarian matching and the DETR set criterion on the device (include/gpv_match.h; the host statements of the same rules are
// gpv1_amd.criterion.lsap_host and match_cost_host).
//
// Solver: ONE WAVE PER PROBLEM, four problems per 256-thread workgroup.  A problem is scipy's rectangular LSAP: shortest augmenting
// paths with float64 duals u, v, on the transposed matrix when there are more rows than columns.  All solver state of a problem lives
// in that wave's slice of LDS; lanes run over the positions of `remaining`, so a search step is: every remaining column's path cost
// updated, one butterfly over (value, tie key), one column removed.  Nothing in the search needs a workgroup barrier: a wave runs its
// LDS operations in order, and wave_sync() only keeps the compiler from moving LDS accesses across the points where lanes exchange data.
// The tie rule is scipy's serial scan restated as a key (lsap_host): among the columns at the minimum the LAST position in `remaining`
// that is unassigned, else the FIRST position.  key = 512 + pos for an unassigned column, 511 - pos otherwise, larger wins.
// Every loop is bounded by a shape: a search takes at most nc steps (each removes a column), a path flip at most nr; a minimum that is
// not < +inf (or a NaN) ends the problem with a status word.
// The cost of gpv_match_boxes is written operation by operation and the file is compiled with -ffp-contract=off, so that the kernel and
// the host rule round the same products and sums.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/gpv_match.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAXD = GPV_MATCH_MAX_DIM;
constexpr int TILE = GPV_MATCH_TILE;
constexpr int WAVES = 4;

struct Prob {                       // 15872 bytes; four of them are 62 KB of LDS per workgroup
    double u[MAXD], v[MAXD], spc[MAXD];
    int path[MAXD], col4row[MAXD], row4col[MAXD], remaining[MAXD];
    unsigned char SR[MAXD], SC[MAXD];
    float tile[TILE];
};

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// cost(i, j) = cb[i * si + j * sj]; cb points into LDS (the tile) or into global memory.  -> status
__device__ int solve(Prob& s, const float* cb, int si, int sj, int nr, int nc, int lane) {
    for (int k = lane; k < MAXD; k += 64) {
        s.u[k] = 0.0;
        s.v[k] = 0.0;
        s.path[k] = -1;
        s.row4col[k] = -1;
        s.col4row[k] = -1;
    }
    wave_sync();
    for (int cur = 0; cur < nr; ++cur) {
        for (int j = lane; j < nc; j += 64) {
            s.remaining[j] = nc - 1 - j;
            s.SC[j] = 0;
            s.spc[j] = INFINITY;
        }
        for (int i = lane; i < nr; i += 64) s.SR[i] = 0;
        wave_sync();
        int i = cur, nrem = nc, sink = -1;
        double minVal = 0.0;
        for (int step = 0; step < nc; ++step) {
            if (lane == 0) s.SR[i] = 1;
            const double ui = s.u[i];
            double bv = INFINITY;
            int bk = -1;
            for (int it = lane; it < nrem; it += 64) {
                const int j = s.remaining[it];
                const double r = ((minVal + (double)cb[(size_t)i * si + (size_t)j * sj]) - ui) - s.v[j];
                double sp = s.spc[j];
                if (r < sp) {
                    s.path[j] = i;
                    s.spc[j] = r;
                    sp = r;
                }
                const int key = s.row4col[j] < 0 ? 512 + it : 511 - it;
                if (sp < bv || (sp == bv && key > bk)) {
                    bv = sp;
                    bk = key;
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double ov = __shfl_xor(bv, off);
                const int ok = __shfl_xor(bk, off);
                if (ov < bv || (ov == bv && ok > bk)) {
                    bv = ov;
                    bk = ok;
                }
            }
            minVal = bv;
            if (!(minVal < (double)INFINITY) || bk < 0) return GPV_MATCH_ERR_INFEASIBLE;
            const int index = clampi(bk >= 512 ? bk - 512 : 511 - bk, 0, nrem - 1);
            wave_sync();
            const int j = clampi(s.remaining[index], 0, nc - 1);
            const int r4 = s.row4col[j];
            const int last = s.remaining[nrem - 1];
            wave_sync();
            if (lane == 0) {
                s.SC[j] = 1;
                s.remaining[index] = last;
            }
            --nrem;
            wave_sync();
            if (r4 < 0) {
                sink = j;
                break;
            }
            i = clampi(r4, 0, nr - 1);
        }
        if (sink < 0) return GPV_MATCH_ERR_INFEASIBLE;
        // dual variables
        for (int r = lane; r < nr; r += 64) {
            if (r == cur) s.u[r] += minVal;
            else if (s.SR[r]) s.u[r] += minVal - s.spc[clampi(s.col4row[r], 0, nc - 1)];
        }
        for (int j = lane; j < nc; j += 64)
            if (s.SC[j]) s.v[j] -= minVal - s.spc[j];
        wave_sync();
        // augment: at most nr rows lie on the path
        if (lane == 0) {
            int j = sink;
            for (int t = 0; t < nr; ++t) {
                const int r = clampi(s.path[clampi(j, 0, nc - 1)], 0, nr - 1);
                s.row4col[clampi(j, 0, nc - 1)] = r;
                const int nj = s.col4row[r];
                s.col4row[r] = j;
                j = nj;
                if (r == cur) break;
            }
        }
        wave_sync();
    }
    return 0;
}

// pairs sorted by prediction; transposed: rows are targets, columns predictions.  -> number of pairs
__device__ int write_pairs(const Prob& s, bool transposed, int nr, int nc, int Kmax, int* pred, int* tgt, int lane) {
    if (!transposed) {
        for (int i = lane; i < nr; i += 64) {
            pred[i] = i;
            tgt[i] = s.col4row[i];
        }
    } else {
        int base = 0;
        for (int j0 = 0; j0 < nc; j0 += 64) {
            const int j = j0 + lane;
            const int r = j < nc ? s.row4col[j] : -1;
            const unsigned long long m = __ballot(r >= 0);
            const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
            if (r >= 0 && pos < Kmax) {
                pred[pos] = j;
                tgt[pos] = r;
            }
            base += __popcll(m);
        }
    }
    for (int k = nr + lane; k < Kmax; k += 64) {
        pred[k] = -1;
        tgt[k] = -1;
    }
    return nr;
}

__device__ void write_none(int Kmax, int* pred, int* tgt, int lane) {
    for (int k = lane; k < Kmax; k += 64) {
        pred[k] = -1;
        tgt[k] = -1;
    }
}

__device__ __forceinline__ bool bad_cost(float c) { return c != c || c == -INFINITY; }

__global__ __launch_bounds__(64 * WAVES) void lsap_kernel(const float* __restrict__ cost, const int* __restrict__ g_count, int P, int Q,
                                                          int Gmax, int Kmax, int* __restrict__ pred_idx, int* __restrict__ tgt_idx,
                                                          int* __restrict__ n_pairs, int* __restrict__ status) {
    __shared__ Prob probs[WAVES];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p = blockIdx.x * WAVES + w;
    if (p >= P) return;
    Prob& s = probs[w];
    int* pred = pred_idx + (size_t)p * Kmax;
    int* tgt = tgt_idx + (size_t)p * Kmax;
    int g = g_count[p];
    g = g < 0 ? 0 : (g > Gmax ? Gmax : g);
    if (g == 0) {
        write_none(Kmax, pred, tgt, lane);
        if (lane == 0) {
            n_pairs[p] = 0;
            status[p] = 0;
        }
        return;
    }
    const float* c = cost + (size_t)p * Q * Gmax;
    const bool transposed = g < Q;
    const int nr = transposed ? g : Q, nc = transposed ? Q : g;
    const bool in_lds = Q * g <= TILE;
    bool bad = false;
    for (int e = lane; e < Q * g; e += 64) {
        const int q = e / g, t = e - q * g;
        const float x = c[(size_t)q * Gmax + t];
        bad |= bad_cost(x);
        if (in_lds) s.tile[transposed ? t * nc + q : q * nc + t] = x;
    }
    int st = __any(bad) ? GPV_MATCH_ERR_INVALID : 0;
    wave_sync();
    if (st == 0) {
        if (in_lds) st = solve(s, s.tile, nc, 1, nr, nc, lane);
        else st = solve(s, c, transposed ? 1 : Gmax, transposed ? Gmax : 1, nr, nc, lane);
    }
    int n = 0;
    if (st == 0) n = write_pairs(s, transposed, nr, nc, Kmax, pred, tgt, lane);
    else write_none(Kmax, pred, tgt, lane);
    if (lane == 0) {
        n_pairs[p] = n;
        status[p] = st;
    }
}

struct Box {
    float x0, y0, x1, y1;
};

__device__ __forceinline__ Box corners(float4 b) {
    Box r;
    r.x0 = b.x - 0.5f * b.z;
    r.y0 = b.y - 0.5f * b.w;
    r.x1 = b.x + 0.5f * b.z;
    r.y1 = b.y + 0.5f * b.w;
    return r;
}

// generalized_box_iou of one pair, fp32, in the order of criterion.generalized_box_iou
__device__ __forceinline__ float giou32(Box a, Box b) {
    const float a1 = (a.x1 - a.x0) * (a.y1 - a.y0), a2 = (b.x1 - b.x0) * (b.y1 - b.y0);
    const float iw = fmaxf(fminf(a.x1, b.x1) - fmaxf(a.x0, b.x0), 0.f), ih = fmaxf(fminf(a.y1, b.y1) - fmaxf(a.y0, b.y0), 0.f);
    const float inter = iw * ih;
    const float uni = (a1 + a2) - inter;
    const float iou = inter / uni;
    const float ew = fmaxf(fmaxf(a.x1, b.x1) - fminf(a.x0, b.x0), 0.f), eh = fmaxf(fmaxf(a.y1, b.y1) - fminf(a.y0, b.y0), 0.f);
    const float area = ew * eh;
    return iou - (area - uni) / area;
}

__global__ __launch_bounds__(64 * WAVES) void match_boxes_kernel(const float* __restrict__ logits, const float4* __restrict__ boxes,
                                                                 const float4* __restrict__ tgt_boxes, const int* __restrict__ tgt_labels,
                                                                 const int* __restrict__ g_count, int L, int B, int Q, int C1, int Gmax,
                                                                 int Kmax, float w_class, float w_bbox, float w_giou, float* cost_out,
                                                                 int* __restrict__ pred_idx, int* __restrict__ tgt_idx,
                                                                 int* __restrict__ n_pairs, int* __restrict__ status) {
    __shared__ Prob probs[WAVES];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p = blockIdx.x * WAVES + w;
    if (p >= L * B) return;
    Prob& s = probs[w];
    const int b = p % B;
    int* pred = pred_idx + (size_t)p * Kmax;
    int* tgt = tgt_idx + (size_t)p * Kmax;
    int g = g_count[b];
    g = g < 0 ? 0 : (g > Gmax ? Gmax : g);
    if (g == 0) {
        write_none(Kmax, pred, tgt, lane);
        if (lane == 0) {
            n_pairs[p] = 0;
            status[p] = 0;
        }
        return;
    }
    const bool transposed = g < Q;
    const int nr = transposed ? g : Q, nc = transposed ? Q : g;
    const bool in_lds = Q * g <= TILE;
    float* c = cost_out ? cost_out + (size_t)p * Q * Gmax : nullptr;
    const float* lg = logits + (size_t)p * Q * C1;
    const float4* pb = boxes + (size_t)p * Q;
    const float4* tb = tgt_boxes + (size_t)b * Gmax;
    const int* tl = tgt_labels + (size_t)b * Gmax;
    bool bad = false, degenerate = false;
    for (int e = lane; e < Q * g; e += 64) {
        const int q = e / g, t = e - q * g;
        const float* x = lg + (size_t)q * C1;
        const int label = tl[t];
        bad |= label < 0 || label >= C1;
        const int lab = clampi(label, 0, C1 - 1);
        float m = x[0];
        for (int k = 1; k < C1; ++k) m = fmaxf(m, x[k]);
        float sum = 0.f, el = 0.f;
        for (int k = 0; k < C1; ++k) {
            const float ex = expf(x[k] - m);
            sum = sum + ex;
            el = k == lab ? ex : el;
        }
        const float prob = el / sum;
        const float4 pq = pb[q], tt = tb[t];
        const float l1 = ((fabsf(pq.x - tt.x) + fabsf(pq.y - tt.y)) + fabsf(pq.z - tt.z)) + fabsf(pq.w - tt.w);
        const Box a = corners(pq), bb = corners(tt);
        degenerate |= a.x1 < a.x0 || a.y1 < a.y0 || bb.x1 < bb.x0 || bb.y1 < bb.y0;
        const float gi = giou32(a, bb);
        const float cst = (w_bbox * l1 + w_class * (-prob)) + w_giou * (-gi);
        bad |= bad_cost(cst);
        if (in_lds) s.tile[transposed ? t * nc + q : q * nc + t] = cst;
        if (c) c[(size_t)q * Gmax + t] = cst;
    }
    int st = (__any(bad) ? GPV_MATCH_ERR_INVALID : 0) | (__any(degenerate) ? GPV_MATCH_ERR_DEGENERATE : 0);
    if (!in_lds) __threadfence();          // this wave reads back what its other lanes wrote to cost_out
    wave_sync();
    int sv = st & GPV_MATCH_ERR_INVALID;
    if (sv == 0) {
        if (in_lds) sv = solve(s, s.tile, nc, 1, nr, nc, lane);
        else sv = solve(s, c, transposed ? 1 : Gmax, transposed ? Gmax : 1, nr, nc, lane);
    }
    int n = 0;
    if (sv == 0) n = write_pairs(s, transposed, nr, nc, Kmax, pred, tgt, lane);
    else write_none(Kmax, pred, tgt, lane);
    if (lane == 0) {
        n_pairs[p] = n;
        status[p] = st | sv;
    }
}

// ------------------------------------------------------------------------------------------------ set criterion
constexpr int LOSS_THREADS = 256;

// d(min(a, b)) / da and d(max(a, b)) / da as torch.min / torch.max give them: one half each on a tie
__device__ __forceinline__ double d_min(double a, double b) { return a < b ? 1.0 : (a == b ? 0.5 : 0.0); }
__device__ __forceinline__ double d_max(double a, double b) { return a > b ? 1.0 : (a == b ? 0.5 : 0.0); }

// giou of src (cxcywh) against tgt and its gradient with respect to src's cx, cy, w, h
__device__ double giou_grad(const double* sb, const double* tb, double* grad) {
    const double x0 = sb[0] - 0.5 * sb[2], y0 = sb[1] - 0.5 * sb[3], x1 = sb[0] + 0.5 * sb[2], y1 = sb[1] + 0.5 * sb[3];
    const double tx0 = tb[0] - 0.5 * tb[2], ty0 = tb[1] - 0.5 * tb[3], tx1 = tb[0] + 0.5 * tb[2], ty1 = tb[1] + 0.5 * tb[3];
    const double aw = x1 - x0, ah = y1 - y0;
    const double a1 = aw * ah, a2 = (tx1 - tx0) * (ty1 - ty0);
    const double iwr = fmin(x1, tx1) - fmax(x0, tx0), ihr = fmin(y1, ty1) - fmax(y0, ty0);
    const double iw = fmax(iwr, 0.0), ih = fmax(ihr, 0.0);
    const double mw = iwr >= 0.0 ? 1.0 : 0.0, mh = ihr >= 0.0 ? 1.0 : 0.0;
    const double inter = iw * ih, uni = (a1 + a2) - inter;
    const double ewr = fmax(x1, tx1) - fmin(x0, tx0), ehr = fmax(y1, ty1) - fmin(y0, ty0);
    const double ew = fmax(ewr, 0.0), eh = fmax(ehr, 0.0);
    const double nw = ewr >= 0.0 ? 1.0 : 0.0, nh = ehr >= 0.0 ? 1.0 : 0.0;
    const double area = ew * eh;
    const double giou = inter / uni - (area - uni) / area;
    const double kI = 1.0 / uni, kU = -inter / (uni * uni) + 1.0 / area, kA = -uni / (area * area);
    // corners: x0, x1, y0, y1
    const double dI_x0 = -ih * mw * d_max(x0, tx0), dI_x1 = ih * mw * d_min(x1, tx1);
    const double dI_y0 = -iw * mh * d_max(y0, ty0), dI_y1 = iw * mh * d_min(y1, ty1);
    const double dA_x0 = -eh * nw * d_min(x0, tx0), dA_x1 = eh * nw * d_max(x1, tx1);
    const double dA_y0 = -ew * nh * d_min(y0, ty0), dA_y1 = ew * nh * d_max(y1, ty1);
    const double g_x0 = kI * dI_x0 + kU * (-ah - dI_x0) + kA * dA_x0;
    const double g_x1 = kI * dI_x1 + kU * (ah - dI_x1) + kA * dA_x1;
    const double g_y0 = kI * dI_y0 + kU * (-aw - dI_y0) + kA * dA_y0;
    const double g_y1 = kI * dI_y1 + kU * (aw - dI_y1) + kA * dA_y1;
    grad[0] = g_x0 + g_x1;
    grad[1] = g_y0 + g_y1;
    grad[2] = 0.5 * (g_x1 - g_x0);
    grad[3] = 0.5 * (g_y1 - g_y0);
    return giou;
}

__global__ __launch_bounds__(LOSS_THREADS) void set_loss_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                                const float* __restrict__ tgt_boxes, const int* __restrict__ tgt_labels,
                                                                const int* __restrict__ g_count, const int* __restrict__ pred_idx,
                                                                const int* __restrict__ tgt_idx, const int* __restrict__ n_pairs, int L,
                                                                int B, int Q, int C1, int Gmax, int Kmax, float eos_coef,
                                                                double* __restrict__ partial, float* __restrict__ dlogits,
                                                                float* __restrict__ dboxes_l1, float* __restrict__ dboxes_giou,
                                                                double* __restrict__ num_boxes, const int* __restrict__ status) {
    __shared__ int s_tgt[MAXD];
    __shared__ double s_sum[4][LOSS_THREADS];
    const int p = blockIdx.x, t = threadIdx.x, b = p % B;
    if (p == 0 && t == 0) {
        long long nb = 0;
        for (int i = 0; i < B; ++i) nb += g_count[i] > 0 ? (g_count[i] > Gmax ? Gmax : g_count[i]) : 0;
        num_boxes[0] = nb < 1 ? 1.0 : (double)nb;
    }
    const int gc = g_count[b];
    const int g = gc < 0 ? 0 : (gc > Gmax ? Gmax : gc);
    const bool q_ok = t < Q;
    const size_t row = (size_t)p * Q + (q_ok ? t : 0);
    if (gc < 0) {                                   // the image takes no part in localisation
        if (q_ok) {
            for (int k = 0; k < C1; ++k) dlogits[row * C1 + k] = 0.f;
            for (int k = 0; k < 4; ++k) dboxes_l1[row * 4 + k] = dboxes_giou[row * 4 + k] = 0.f;
        }
        if (t < 4) partial[(size_t)p * 4 + t] = 0.0;
        return;
    }
    if (q_ok) s_tgt[t] = -1;
    __syncthreads();
    int np = n_pairs[p];
    np = np < 0 ? 0 : (np > Kmax ? Kmax : np);
    for (int k = t; k < np; k += LOSS_THREADS) {
        const int q = pred_idx[(size_t)p * Kmax + k], j = tgt_idx[(size_t)p * Kmax + k];
        if (q >= 0 && q < Q && j >= 0 && j < g) s_tgt[q] = j;      // pred indices of a problem are distinct: no two writers of a slot
    }
    __syncthreads();
    double v_num = 0.0, v_den = 0.0, v_l1 = 0.0, v_gi = 0.0;
    if (q_ok) {
        const int j = s_tgt[t];
        const float* x = logits + row * C1;
        const int cls = j >= 0 ? clampi(tgt_labels[(size_t)b * Gmax + j], 0, C1 - 1) : C1 - 1;
        const double wt = cls == C1 - 1 ? (double)eos_coef : 1.0;
        double m = (double)x[0];
        for (int k = 1; k < C1; ++k) m = fmax(m, (double)x[k]);
        double sum = 0.0;
        for (int k = 0; k < C1; ++k) sum += exp((double)x[k] - m);
        const double lse = m + log(sum);
        v_num = wt * (lse - (double)x[cls]);
        v_den = wt;
        for (int k = 0; k < C1; ++k) dlogits[row * C1 + k] = (float)(wt * (exp((double)x[k] - lse) - (k == cls ? 1.0 : 0.0)));
        double gl1[4] = {0.0, 0.0, 0.0, 0.0}, ggi[4] = {0.0, 0.0, 0.0, 0.0};
        if (j >= 0) {
            double sb[4], tb[4];
            for (int k = 0; k < 4; ++k) {
                sb[k] = (double)boxes[row * 4 + k];
                tb[k] = (double)tgt_boxes[((size_t)b * Gmax + j) * 4 + k];
                const double d = sb[k] - tb[k];
                v_l1 += fabs(d);
                gl1[k] = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
            }
            v_gi = 1.0 - giou_grad(sb, tb, ggi);
            for (int k = 0; k < 4; ++k) ggi[k] = -ggi[k];
        }
        for (int k = 0; k < 4; ++k) {
            dboxes_l1[row * 4 + k] = (float)gl1[k];
            dboxes_giou[row * 4 + k] = (float)ggi[k];
        }
    }
    s_sum[0][t] = v_num;
    s_sum[1][t] = v_den;
    s_sum[2][t] = v_l1;
    s_sum[3][t] = v_gi;
    __syncthreads();
    for (int h = LOSS_THREADS / 2; h >= 1; h >>= 1) {      // fixed tree: the same order on every run
        if (t < h)
            for (int k = 0; k < 4; ++k) s_sum[k][t] += s_sum[k][t + h];
        __syncthreads();
    }
    if (t < 4) partial[(size_t)p * 4 + t] = status[p] != 0 ? (double)NAN : s_sum[t][0];
}

bool shapes_ok(int Q, int Gmax, int Kmax) {
    return Q >= 1 && Q <= MAXD && Gmax >= 1 && Gmax <= MAXD && Kmax >= (Q < Gmax ? Q : Gmax);
}

}  // namespace

extern "C" int gpv_match_lsap(const float* cost, const int* g_count, int P, int Q, int Gmax, int Kmax, int* pred_idx, int* tgt_idx,
                              int* n_pairs, int* status, void* stream) {
    if (P < 0 || !shapes_ok(Q, Gmax, Kmax)) return (int)hipErrorInvalidValue;
    if (P == 0) return (int)hipSuccess;
    if (!cost || !g_count || !pred_idx || !tgt_idx || !n_pairs || !status) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lsap_kernel, dim3((P + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, (hipStream_t)stream, cost, g_count, P, Q, Gmax, Kmax,
                       pred_idx, tgt_idx, n_pairs, status);
    return (int)hipGetLastError();
}

extern "C" int gpv_match_boxes(const float* logits, const float* boxes, const float* tgt_boxes, const int* tgt_labels, const int* g_count,
                               int L, int B, int Q, int C1, int Gmax, int Kmax, float w_class, float w_bbox, float w_giou, float* cost_out,
                               int* pred_idx, int* tgt_idx, int* n_pairs, int* status, void* stream) {
    if (L < 0 || B < 0 || !shapes_ok(Q, Gmax, Kmax) || C1 < 2 || C1 > GPV_MATCH_MAX_CLASSES) return (int)hipErrorInvalidValue;
    if ((long long)L * B > (1LL << 24)) return (int)hipErrorInvalidValue;
    if (L * B == 0) return (int)hipSuccess;
    if (!logits || !boxes || !tgt_boxes || !tgt_labels || !g_count || !pred_idx || !tgt_idx || !n_pairs || !status)
        return (int)hipErrorInvalidValue;
    if (!cost_out && Q * Gmax > TILE) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(tgt_boxes)) & 15) return (int)hipErrorInvalidValue;   // float4 loads
    hipLaunchKernelGGL(match_boxes_kernel, dim3((L * B + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, (hipStream_t)stream, logits,
                       reinterpret_cast<const float4*>(boxes), reinterpret_cast<const float4*>(tgt_boxes), tgt_labels, g_count, L, B, Q, C1,
                       Gmax, Kmax, w_class, w_bbox, w_giou, cost_out, pred_idx, tgt_idx, n_pairs, status);
    return (int)hipGetLastError();
}

extern "C" int gpv_match_set_loss(const float* logits, const float* boxes, const float* tgt_boxes, const int* tgt_labels, const int* g_count,
                                  const int* pred_idx, const int* tgt_idx, const int* n_pairs, int L, int B, int Q, int C1, int Gmax,
                                  int Kmax, float eos_coef, double* partial, float* dlogits, float* dboxes_l1, float* dboxes_giou,
                                  double* num_boxes, const int* status, void* stream) {
    if (L < 0 || B < 0 || Q < 1 || Q > MAXD || Gmax < 1 || Gmax > MAXD || Kmax < 1 || C1 < 2 || C1 > GPV_MATCH_MAX_CLASSES)
        return (int)hipErrorInvalidValue;
    if ((long long)L * B > (1LL << 24)) return (int)hipErrorInvalidValue;
    if (L * B == 0) return (int)hipSuccess;
    if (!logits || !boxes || !tgt_boxes || !tgt_labels || !g_count || !pred_idx || !tgt_idx || !n_pairs || !partial || !dlogits ||
        !dboxes_l1 || !dboxes_giou || !num_boxes || !status)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(set_loss_kernel, dim3(L * B), dim3(LOSS_THREADS), 0, (hipStream_t)stream, logits, boxes, tgt_boxes, tgt_labels,
                       g_count, pred_idx, tgt_idx, n_pairs, L, B, Q, C1, Gmax, Kmax, eos_coef, partial, dlogits, dboxes_l1, dboxes_giou,
                       num_boxes, status);
    return (int)hipGetLastError();
}
