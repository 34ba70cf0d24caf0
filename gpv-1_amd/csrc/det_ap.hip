// Per-sample detection AP on the device (include/gpv_eval.h gpv_eval_det_ap; the host statement of the same rule is
// gpv1_amd.evaluators.det_ap_host).  One workgroup per sample, thread r owns query r and later sorted position r; no atomics, nothing
// crosses a workgroup.  Phases (a barrier between each):
//   1 score   thread q: softmax(logit pair)[0] in fp32, key = the score's bits made monotone (a total order even for a NaN)
//   2 sort    rank of q = #{j : key_j > key_q or (key_j == key_q and j < q)}: the index is part of the key, so ranks are a
//             permutation and equal scores keep query order (stable descending).  O(Q^2 / threads) LDS broadcasts: 100 for Q = 100
//   3 match   the sorted boxes and (up to GT_LDS of) the ground-truth boxes are staged in LDS first: the loop below then has no global
//             load on its dependent chain (box -> ground truth -> IoU cost two memory latencies per detection, 25 detections per wave).
//             One WAVE per sorted detection, lanes over the ground-truth boxes (a loop when there are more than 64): each lane keeps
//             its first largest IoU > 0, a butterfly picks the largest of the wave, the lowest box index among equals
//   4 taken   a box is taken by the FIRST detection in order whose candidate it is with IoU >= thresh, so position r is a true
//             positive iff no earlier position has the same candidate over the threshold: the sequential walk's taken-mask without
//             the walk and without a mask (any G fits)
//   5 counts  tp_r = #true positives up to r; prec_r = tp_r / (r + 1) in fp64
//   6 terms   at a true positive recall steps from (tp_r - 1) / npos to tp_r / npos: term = step * max_{j >= r} prec_j
//   7 sum     thread 0 adds the terms in order (the host adds the same numbers in the same order; the zeros in between are exact)
// The IoU is written operation by operation and the file is compiled with -ffp-contract=off: a fused multiply-add would round
// aw*ah + bw*bh once instead of twice and could move a decision at the threshold away from the host rule's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/gpv_eval.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAXQ = GPV_EVAL_MAX_Q;
constexpr int GT_LDS = 256;      // ground-truth boxes of a sample kept in LDS (more: read from global memory, L1 / L2 hits)

__device__ __forceinline__ unsigned order_key(float s) {
    unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(1024) void det_ap_kernel(const float* __restrict__ rel_logits, const float* __restrict__ boxes,
                                                      const float* __restrict__ gt, const int* __restrict__ gt_count, int Q, int G,
                                                      float iou_thresh, float* __restrict__ score, int* __restrict__ order,
                                                      unsigned char* __restrict__ tp, double* __restrict__ ap) {
    __shared__ unsigned s_key[MAXQ];
    __shared__ float s_score[MAXQ];
    __shared__ int s_order[MAXQ];
    __shared__ int s_cand[MAXQ];
    __shared__ float s_iou[MAXQ];
    __shared__ int s_tp[MAXQ];
    __shared__ double s_prec[MAXQ];
    __shared__ double s_term[MAXQ];
    __shared__ float4 s_box[MAXQ];
    __shared__ float4 s_gt[GT_LDS];
    const int b = blockIdx.x, t = threadIdx.x;
    const size_t row = (size_t)b * Q;
    int npos = gt_count[b];
    npos = npos < 0 ? 0 : (npos > G ? G : npos);

    float sc = 0.f;
    unsigned key = 0;
    if (t < Q) {
        const float l0 = rel_logits[(row + t) * 2], l1 = rel_logits[(row + t) * 2 + 1];
        const float m = fmaxf(l0, l1);
        const float e0 = expf(l0 - m), e1 = expf(l1 - m);
        sc = e0 / (e0 + e1);
        key = order_key(sc);
        s_key[t] = key;
    }
    __syncthreads();

    if (t < Q) {
        int rank = 0;
        for (int j = 0; j < Q; ++j) {
            const unsigned kj = s_key[j];
            rank += (kj > key || (kj == key && j < t)) ? 1 : 0;
        }
        s_score[rank] = sc;
        s_order[rank] = t;
    }
    __syncthreads();

    if (t < Q) {
        score[row + t] = s_score[t];
        order[row + t] = s_order[t];
        s_box[t] = *reinterpret_cast<const float4*>(boxes + (row + s_order[t]) * 4);
    }
    const bool gt_in_lds = npos <= GT_LDS;
    if (gt_in_lds)
        for (int g = t; g < npos; g += blockDim.x) s_gt[g] = *reinterpret_cast<const float4*>(gt + ((size_t)b * G + g) * 4);
    __syncthreads();

    const int lane = t & 63, nwave = blockDim.x >> 6;
    for (int r = t >> 6; r < Q; r += nwave) {
        const float4 p = s_box[r];
        const float aw = p.z, ah = p.w;
        const float ax1 = p.x - 0.5f * aw, ay1 = p.y - 0.5f * ah;
        const float ax2 = ax1 + aw, ay2 = ay1 + ah;
        const float aarea = aw * ah;
        float best = 0.f;
        int bg = -1;
        for (int g = lane; g < npos; g += 64) {
            const float4 q = gt_in_lds ? s_gt[g] : *reinterpret_cast<const float4*>(gt + ((size_t)b * G + g) * 4);
            const float bx2 = q.x + q.z, by2 = q.y + q.w;
            const float iw = fmaxf(0.f, fminf(ax2, bx2) - fmaxf(ax1, q.x));
            const float ih = fmaxf(0.f, fminf(ay2, by2) - fmaxf(ay1, q.y));
            const float inter = iw * ih;
            const float barea = q.z * q.w;
            const float uni = (aarea + barea) - inter;
            const float v = uni > 0.f ? inter / uni : 0.f;
            if (v > best) {
                best = v;
                bg = g;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ob = __shfl_xor(best, off, 64);
            const int og = __shfl_xor(bg, off, 64);
            if (ob > best || (ob == best && og >= 0 && og < bg)) {
                best = ob;
                bg = og;
            }
        }
        if (lane == 0) {
            s_cand[r] = bg;
            s_iou[r] = best;
        }
    }
    __syncthreads();

    int hit = 0;
    if (t < Q) {
        const int c = s_cand[t];
        hit = (c >= 0 && s_iou[t] >= iou_thresh) ? 1 : 0;
        for (int j = 0; hit && j < t; ++j)
            if (s_cand[j] == c && s_iou[j] >= iou_thresh) hit = 0;
        s_tp[t] = hit;
        tp[row + t] = (unsigned char)hit;
    }
    __syncthreads();

    int ctp = 0;
    if (t < Q) {
        for (int j = 0; j <= t; ++j) ctp += s_tp[j];
        s_prec[t] = (double)ctp / (double)(t + 1);
    }
    __syncthreads();

    if (t < Q) {
        double term = 0.0;
        if (hit) {
            double env = 0.0;
            for (int j = t; j < Q; ++j) env = fmax(env, s_prec[j]);
            const double rec = (double)ctp / (double)npos, prev = (double)(ctp - 1) / (double)npos;
            term = (rec - prev) * env;
        }
        s_term[t] = term;
    }
    __syncthreads();

    if (t == 0) {
        double acc = 0.0;
        for (int r = 0; r < Q; ++r) acc += s_term[r];
        ap[b] = npos > 0 ? acc : 0.0;
    }
}

}  // namespace

extern "C" int gpv_eval_det_ap(const float* rel_logits, const float* boxes, const float* gt, const int* gt_count, int B, int Q, int G,
                               float iou_thresh, float* score, int* order, unsigned char* tp, double* ap, void* stream) {
    if (B < 0 || Q < 1 || Q > MAXQ || G < 0 || !(iou_thresh == iou_thresh)) return (int)hipErrorInvalidValue;
    if (B == 0) return (int)hipSuccess;
    if (!rel_logits || !boxes || !gt_count || !score || !order || !tp || !ap || (G > 0 && !gt)) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(gt)) & 15) return (int)hipErrorInvalidValue;   // float4 loads
    // thread r owns query r; past that, more waves only shorten the match loop (one detection per wave and turn): 16 waves from Q = 65 up
    const int threads = Q > 64 ? 1024 : 256;
    hipLaunchKernelGGL(det_ap_kernel, dim3(B), dim3(threads), 0, (hipStream_t)stream, rel_logits, boxes, gt, gt_count, Q, G, iou_thresh,
                       score, order, tp, ap);
    return (int)hipGetLastError();
}
