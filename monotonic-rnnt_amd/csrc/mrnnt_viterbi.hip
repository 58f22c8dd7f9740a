// mrnnt_viterbi.hip -- best-path (Viterbi) alignment over the monotonic lattice (mrnnt_align, include/mrnnt.h). The
// reference has no counterpart; the output is the alignment format its restrict_to_alignment parses
// (gpu_workspace_manager.h:191-219). One workgroup per utterance, one launch:
//   1. the max-plus twin of alpha_pass (mrnnt_recursion.hip), same lanes, band and prefetch:
//        v(t, s) = max(v(t-1, s) + lpb(t, s), v(t-1, s-1) + lpe(t, s-1)),  v(-1, s) = [s == 0 ? 0 : -inf]
//      in fp64, recording one back-pointer bit per cell (1: the label arc was taken). Tie rule: the label arc is taken
//      only when it is strictly greater than the blank arc. A NaN arc makes the cell NaN (as the log-sum-exp would).
//   2. after a workgroup barrier, wave 0 walks the bits back from (T-1, S) and stores the alignment row.
//
// Back-pointer bits live in the utterance's own region of the workspace alpha array, which this call does not
// otherwise use: frame t owns the W = S+1 doubles at alpha + row_off + t*W, read as 64-bit words. With K cells per
// lane, cell s sits in lane q = s / K (of the whole workgroup), slot k = s % K, and its bit is
//     word (q / 64) * K + k,  bit q % 64
// of the frame -- word (wave, k) is the wave's ballot over slot k. A word's index never exceeds the lowest cell it
// covers, so every word that holds a cell s < W has an index < W: the frame's W doubles always have room, and only
// words with an index < W are stored or read.
#include "mrnnt_dp.h"

namespace mrnnt {

typedef unsigned long long u64;

constexpr int kBtFrames = 64;            // frames per backtrace chunk: one lane per frame
constexpr int kBtWords = 8 * 4;          // most bit words per frame (8 waves x 4 cells per lane)
constexpr int kBtPitch = kBtWords + 1;   // LDS row pitch (odd: lanes staging one word each hit distinct banks)

template <int K, int D, int NW, bool BAND>
__device__ __forceinline__ void viterbi_pass(const DevProblem &p, int b, double (*xb)[8], double *fin) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int T = p.T[b], S = p.S[b], W = S + 1;
    const int64_t r0 = p.row_off[b], c0 = p.col_off[b];
    const int s0 = (wave * 64 + lane) * K;
    constexpr bool band = BAND;
    static_assert(NW == 1 || NW == 2 || NW == 4 || NW == 8, "cross-wave slots sized for <= 8 waves");
    static_assert(NW * K <= kBtWords, "backtrace staging sized for <= 32 words per frame");

    double a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = (s0 + k == 0) ? 0.0 : NEG_INF_D;
    if (NW > 1 && lane == 0) xb[1][wave] = NEG_INF_D;  // v(-1, s) for the cross-wave neighbour of step 0

    double pb[D][K], pe[D][K];
    int mn[D], mx[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const int tt = min(d, T - 1);
        const Lp *rl = p.lp + r0 + (int64_t)tt * W + s0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            pb[d][k] = rl[k].b;
            pe[d][k] = (s0 + k == 0) ? 0.0 : rl[k - 1].e;  // cell 0 has no s - 1 (see the step's reload)
        }
        mn[d] = band ? p.min_s[c0 + tt] : 0;
        mx[d] = band ? p.max_s[c0 + tt] : S;
    }
    __syncthreads();

    u64 *bits = reinterpret_cast<u64 *>(p.alpha + r0);
    for (int t0 = 0; t0 < T; t0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int t = t0 + d;
            if (t >= T) break;
            const int lo = max(max(t - (T - 1 - S), mn[d]), 0);
            const int hi = min(min(t + 1, S), mx[d]);
            double carry = dpp_shr1(a[K - 1]);
            if (lane == 0) carry = (NW == 1 || wave == 0) ? NEG_INF_D : xb[(t + 1) & 1][wave - 1];
            double na[K];
            u64 m[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int s = s0 + k;
                const double am1 = (k == 0) ? carry : a[k - 1];
                const double x = a[k] + pb[d][k];   // blank arc
                const double y = am1 + pe[d][k];    // label arc (cell 0: -inf)
                const bool in = s >= lo && s <= hi;
                const bool take = y > x || y != y;  // strictly greater; a NaN label arc must not be dropped
                na[k] = in ? (take ? y : x) : NEG_INF_D;
                m[k] = __ballot(in && take);
            }
#pragma unroll
            for (int k = 0; k < K; ++k) a[k] = na[k];
            if (lane < K) {  // lane k stores the wave's word of slot k
                u64 w = m[0];
#pragma unroll
                for (int k = 1; k < K; ++k) w = (lane == k) ? m[k] : w;
                const int wi = wave * K + lane;
                if (wi < W) bits[(int64_t)t * W + wi] = w;
            }
            if (NW > 1 && lane == 63) xb[t & 1][wave] = na[K - 1];
            const int tn = min(t + D, T - 1);
            const Lp *rl = p.lp + r0 + (int64_t)tn * W + s0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                pb[d][k] = rl[k].b;
                // as alpha_pass: cell 0's label term is -inf whatever rl[-1] (the row before this frame's) holds
                pe[d][k] = (s0 + k == 0) ? 0.0 : rl[k - 1].e;
            }
            mn[d] = band ? p.min_s[c0 + tn] : 0;
            mx[d] = band ? p.max_s[c0 + tn] : S;
            if (NW > 1) __syncthreads();
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (s0 + k == S) *fin = a[k];
}

// Backtrace, one wave, from (T-1, S) down to frame 0. The bit words are staged through LDS in chunks of 64 frames
// (lane f loads the words of frame tb + f: a few independent loads per lane and chunk, not one dependent global load
// per frame), the walk itself reads only LDS, and lane f keeps the label position frame tb + f emitted, so the chunk's
// alignment entries go out as one store (the labels are gathered after the walk, off its dependent chain).
template <int K, int NW>
__device__ __forceinline__ void backtrace(const DevProblem &p, int b, double fin, int *__restrict__ out,
                                          int64_t out_stride, float *__restrict__ costs, u64 (*bt)[kBtPitch]) {
    const int lane = threadIdx.x & 63;
    const int T = p.T[b], S = p.S[b], W = S + 1;
    int *row = out + (int64_t)b * out_stride;
    if (costs && lane == 0) costs[b] = (float)(-fin);  // -inf: no finite path (+inf cost); NaN stays NaN
    if (!(fin - fin == 0.0)) {                          // not finite: the whole row is -1
        for (int64_t t = lane; t < out_stride; t += 64) row[t] = -1;
        return;
    }
    for (int64_t t = (int64_t)T + lane; t < out_stride; t += 64) row[t] = p.blank;
    const int nw = min(W, NW * K);
    const u64 *bits = reinterpret_cast<const u64 *>(p.alpha + p.row_off[b]);
    const int *lab = p.labels + (int64_t)b * p.label_stride;
    int s = S;
    for (int tb = ((T - 1) / kBtFrames) * kBtFrames; tb >= 0; tb -= kBtFrames) {
        const int t = tb + lane;
        if (t < T) {
            const u64 *src = bits + (int64_t)t * W;
#pragma unroll 4
            for (int j = 0; j < nw; ++j) bt[lane][j] = src[j];
        }
        // one wave: its LDS accesses complete in order; keep the compiler from moving the reads above the writes
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        int my = 0;
        for (int f = min(kBtFrames - 1, T - 1 - tb); f >= 0; --f) {
            const int q = s / K, k = s - q * K;
            const u64 word = bt[f][(q >> 6) * K + k];
            // (cell 0 never takes the label arc; the guard keeps s >= 0 whatever a word holds)
            const int bit = __builtin_amdgcn_readfirstlane((int)((word >> (q & 63)) & 1)) & (s > 0 ? 1 : 0);
            if (lane == f) my = bit ? s : 0;  // emitted label s - 1 (s >= 1), or blank
            s -= bit;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (t < T) row[t] = my > 0 ? lab[my - 1] : p.blank;
    }
}

template <int K, int D, int NW, bool BAND>
__global__ __launch_bounds__(64 * NW) void viterbi_kernel(DevProblem p, int *__restrict__ out, int64_t out_stride,
                                                          float *__restrict__ costs) {
    __shared__ double xb[2][8];
    __shared__ double fin;
    __shared__ u64 bt[kBtFrames][kBtPitch];
    const int b = (int)blockIdx.x;
    // device-resident lengths that failed validation: the lengths may be anything, so no lattice array is touched
    if (p.dyn && __builtin_amdgcn_readfirstlane(p.dyn->status)) {
        int *row = out + (int64_t)b * out_stride;
        for (int64_t t = threadIdx.x; t < out_stride; t += 64 * NW) row[t] = -1;
        if (costs && threadIdx.x == 0) costs[b] = __builtin_nanf("");
        return;
    }
    viterbi_pass<K, D, NW, BAND>(p, b, xb, &fin);
    __syncthreads();  // the bit words (global) and fin (LDS) of every wave are visible to wave 0
    if (threadIdx.x >= 64) return;
    backtrace<K, NW>(p, b, fin, out, out_stride, costs, bt);
}

struct ViterbiLaunch {  // launch_by_width's go<K, NW>() for viterbi_kernel
    const DevProblem &p;
    int *out;
    int64_t out_stride;
    float *costs;
    hipStream_t stream;
    template <int K, int NW>
    void go() const {
        constexpr int D = K <= 2 ? 8 : 4;  // lp rows prefetched ahead, as DpLaunch (mrnnt_recursion.hip)
        if (p.min_s)
            viterbi_kernel<K, D, NW, true><<<p.B, 64 * NW, 0, stream>>>(p, out, out_stride, costs);
        else
            viterbi_kernel<K, D, NW, false><<<p.B, 64 * NW, 0, stream>>>(p, out, out_stride, costs);
    }
};

// one wave (no barrier in the step) up to 64 cells, then as the recursion (launch_by_width, mrnnt_dp.h)
hipError_t launch_viterbi(const DevProblem &p, int S_max, int *out, int64_t out_stride, float *costs,
                          hipStream_t stream) {
    if (!launch_by_width<true>(S_max + 1, ViterbiLaunch{p, out, out_stride, costs, stream})) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace mrnnt
