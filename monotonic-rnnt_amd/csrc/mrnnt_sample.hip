// mrnnt_sample.hip -- whole alignments drawn from the path posterior p(path | labels, acts) (mrnnt_sample,
// include/mrnnt.h): a read-out over the workspace of mrnnt_forward(with_beta = 1), like mrnnt_posterior.hip. A walker
// starts at s = 0 before frame 0 and goes forward in time; standing on row (t, s) it takes the label arc with
//   p_label = 1 / (1 + exp(x - y)),  x = lpb(t, s) + beta(t+1, s),  y = lpe(t, s) + beta(t+1, s+1)
// (sample_p_label, mrnnt_sample.h; beta(T, s) = [s == S]) when u(b, k, t) < p_label, u from Philox4x32-10 keyed by the
// seed and counted by (t >> 2, sample, b) -- so a sample depends on (seed, b, sample index, t) and the state only.
// It reads lp / beta / ll, the labels and the lengths: no acts, no alpha.
//
// Which rows are read. A walker only stands on reachable rows, whose lp the forward wrote and whose successors'
// beta is trustworthy, with one exception decided by index arithmetic: the blank arc that would leave the monotonic
// band (T-1-t < S-s) is -inf without a read (the lean recursion leaves finite values there, mrnnt_setup.hip).
// Everything read AHEAD of a walker (the staging below) may be uninitialised memory -- rows outside an alignment
// window are never written -- and is used only if the walker arrives there, when it is a reachable row after all.
//
// One wave per (utterance, 64 samples); lanes are samples, so neighbouring lanes stand on neighbouring or identical
// rows (paths cluster around the posterior mode). Frames go in chunks of kFrames = 16:
//   1. stage: with [s_lo, s_hi] the wave's range of s at the chunk's first frame, frame f of the chunk can only be
//      met at s_lo <= s <= s_hi + f. p_label of those rows (at most kWin per frame) is computed by all lanes in
//      parallel -- branch-free loads, kStage rows per lane in flight, the fp64 exp off the walk's chain -- into LDS:
//      16 x 96 x 8 B = 12 KiB.
//   2. walk: 16 steps whose dependent chain is one LDS read, a compare and an add; one Philox block per 4 frames,
//      computed a chunk ahead under the latency of the emit loads. A
//      lane outside the staged window (s - s_lo >= kWin: samples spread wider than the window) forms its p_label from
//      global memory with the same function, so the result does not depend on who shares the wave.
//   3. emit: the chunk's 16 decisions sit in a bit mask; the labels are gathered, the chosen arcs' lp (for the path
//      cost, fp64, frame order) loaded and the 16 alignment entries stored (16-byte stores where the row allows)
//      after the walk, as independent accesses.
// No chain of T dependent global round trips: T / 16 stage-walk-emit rounds. One wave is its own workgroup, so the
// __syncthreads() between the phases orders that wave's LDS traffic and waits for nobody. 131 VGPRs, no scratch.
#include "mrnnt_device.h"
#include "mrnnt_sample.h"

namespace mrnnt {

namespace {

constexpr int kFrames = 16;  // frames per chunk: whole Philox blocks (a multiple of 4), one mask bit each
constexpr int kWin = 96;     // staged label positions per frame
constexpr int kStage = 4;    // rows a lane stages per pass, their loads issued together

typedef int i4 __attribute__((ext_vector_type(4)));

// The two arcs out of row (t, s), 0 <= t < T, 0 <= s <= S: x = lpb + beta(t+1, s), y = lpe + beta(t+1, s+1) with the
// boundary rules of the header. Branch-free, so that the loads of several rows issue together: a beta cell that is
// not used (the last frame, a blank arc out of the band, s = S) is read at the row itself instead -- any such row is
// inside the utterance's lattice arrays, and so are (t+1, s) and (t+1, s+1) when t < T-1 and s < S.
struct Arcs {
    double x, y;
};

__device__ __forceinline__ Arcs row_arcs(const DevProblem &p, int64_t r0, int t, int T, int S, int s) {
    const int W = S + 1;
    const int64_t row = r0 + (int64_t)t * W + s;
    const bool last = t == T - 1;
    const bool blank_ok = T - 1 - t >= S - s;  // (last frame: s == S)
    const bool label_ok = s < S;
    const Lp l = p.lp[row];
    const double b1 = p.beta[(last || !blank_ok) ? row : row + W];
    const double b2 = p.beta[(last || !label_ok) ? row : row + W + 1];
    Arcs a;
    a.x = blank_ok ? l.b + (last ? 0.0 : b1) : NEG_INF_D;
    a.y = label_ok ? l.e + (last ? (s + 1 == S ? 0.0 : NEG_INF_D) : b2) : NEG_INF_D;
    return a;
}

__device__ __forceinline__ double row_p_label(const DevProblem &p, int64_t r0, int t, int T, int S, int s) {
    const Arcs a = row_arcs(p, r0, t, T, S, s);
    return sample_p_label(a.x, a.y);
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off));
    return __builtin_amdgcn_readfirstlane(v);
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off));
    return __builtin_amdgcn_readfirstlane(v);
}

// every entry of the wave's nk rows = v, their path costs = c
__device__ __forceinline__ void fill_rows(int *rows, int64_t stride, int nk, int v, float *costs, float c) {
    const int lane = threadIdx.x;
    for (int kk = 0; kk < nk; ++kk)
        for (int64_t t = lane; t < stride; t += 64) rows[kk * stride + t] = v;
    if (costs && lane < nk) costs[lane] = c;
}

__global__ __launch_bounds__(64) void sample_kernel(DevProblem p, SampleArgs a) {
    __shared__ double pl[kFrames][kWin];
    const int lane = threadIdx.x;
    const int nkb = (a.num_samples + 63) / 64;
    const int b = (int)(blockIdx.x / (unsigned)nkb);
    const int k0 = (int)(blockIdx.x - (unsigned)b * nkb) * 64;
    const int nk = min(64, a.num_samples - k0);
    const bool mine = lane < nk;
    // lanes past the last sample walk the last sample again (no special case in the wave's range) and store nothing
    const int k = k0 + min(lane, nk - 1);
    int *rows = a.out + ((int64_t)b * a.num_samples + k0) * a.out_stride;
    float *costs = a.costs ? a.costs + (int64_t)b * a.num_samples + k0 : nullptr;
    const float nan = __builtin_nanf("");
    // device-resident lengths that failed validation: the lengths may be anything, so no lattice array is touched
    if (p.dyn && __builtin_amdgcn_readfirstlane(p.dyn->status)) {
        fill_rows(rows, a.out_stride, nk, -1, costs, nan);
        return;
    }
    const int T = p.T[b], S = p.S[b], W = S + 1;
    if (T > a.out_stride) {  // (device-resident lengths only: the host checks its own) nothing past the stride
        if (k0 == 0 && lane == 0 && p.status_host)
            __hip_atomic_store(p.status_host, (int)RNNT_STATUS_INVALID_VALUE, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        fill_rows(rows, a.out_stride, nk, -1, costs, nan);
        return;
    }
    const double ll = p.ll[b];
    if (!__builtin_isfinite(ll)) {  // -inf: no path (+inf cost); NaN / +inf: NaN
        fill_rows(rows, a.out_stride, nk, -1, costs, ll == NEG_INF_D ? __builtin_huge_valf() : nan);
        return;
    }
    const int64_t r0 = p.row_off[b];
    const int *__restrict__ lab = p.labels + (int64_t)b * p.label_stride;
    int *__restrict__ row = rows + (int64_t)min(lane, nk - 1) * a.out_stride;
    const bool vec_ok = ((reinterpret_cast<uintptr_t>(a.out) | (uintptr_t)(a.out_stride * 4)) & 15) == 0;
    const uint32_t smp = (uint32_t)(a.first_sample + k);
    int s = 0;
    double cost = 0.0;
    // the chunk's random words, four Philox blocks: computed a chunk ahead, under the latency of the emit loads
    uint32_t w[kFrames];
#pragma unroll
    for (int q = 0; q < kFrames / 4; ++q) sample_block(a.seed, (uint32_t)q, smp, (uint32_t)b, w + 4 * q);
    for (int t0 = 0; t0 < T; t0 += kFrames) {
        const int nf = min(kFrames, T - t0);
        // 1. stage p_label of the rows the wave can meet in this chunk
        const int s_lo = wave_min(s), s_hi = wave_max(s);
        const int nw = min(kWin, min(S, s_hi + nf - 1) - s_lo + 1);
        for (int i0 = lane; i0 < nf * nw; i0 += 64 * kStage) {
            Arcs arc[kStage];
            int at[kStage];
#pragma unroll
            for (int u = 0; u < kStage; ++u) {  // kStage rows' loads in flight together (an unused slot: row (t0, s_lo))
                const int i = i0 + 64 * u;
                const int f = i / nw, j = i - f * nw;
                const bool on = i < nf * nw && s_lo + j <= s_hi + f;
                at[u] = on ? f * kWin + j : -1;
                arc[u] = row_arcs(p, r0, t0 + (on ? f : 0), T, S, s_lo + (on ? j : 0));
            }
#pragma unroll
            for (int u = 0; u < kStage; ++u)
                if (at[u] >= 0) (&pl[0][0])[at[u]] = sample_p_label(arc[u].x, arc[u].y);
        }
        __syncthreads();  // (one wave)
        // 2. walk
        const int s_first = s;
        unsigned mask = 0;
#pragma unroll
        for (int f = 0; f < kFrames; ++f) {
            if (f < nf) {
                const int j = s - s_lo;
                double pv;
                if (j < nw) pv = pl[f][j];
                else pv = row_p_label(p, r0, t0 + f, T, S, s);
                const bool take = (sample_uniform(w[f]) < pv) && s < S;
                mask |= (take ? 1u : 0u) << f;
                s += take ? 1 : 0;
            }
        }
        __syncthreads();  // the next chunk's staging overwrites pl
        // 3. emit: labels, the chosen arcs' lp and the chunk's alignment entries. Branch-free loads (a frame past the
        // utterance reads the chunk's first row, a blank frame reads the utterance's own length word in place of a
        // label: valid addresses, values unused), so that all of them are in flight together.
        int v[kFrames];
        double lpv[kFrames];
        int pos = s_first;
#pragma unroll
        for (int f = 0; f < kFrames; ++f) {
            const int bit = (mask >> f) & 1;  // (0 for f >= nf)
            const int ff = f < nf ? f : 0;
            const double *arc = reinterpret_cast<const double *>(p.lp + r0 + (int64_t)(t0 + ff) * W + (f < nf ? pos : s_first));
            lpv[f] = arc[bit];  // Lp = {b, e}
            const int *src = bit ? lab + pos : p.T + b;
            v[f] = *src;
            pos += bit;
        }
#pragma unroll
        for (int q = 0; q < kFrames / 4; ++q)  // the next chunk's random words
            sample_block(a.seed, (uint32_t)((t0 + kFrames) >> 2) + q, smp, (uint32_t)b, w + 4 * q);
#pragma unroll
        for (int f = 0; f < kFrames; ++f) {
            cost += f < nf ? lpv[f] : 0.0;
            v[f] = ((mask >> f) & 1) ? v[f] : p.blank;
        }
        if (mine) {
            if (vec_ok && t0 + kFrames <= a.out_stride) {  // (frames past T inside the chunk: blank)
#pragma unroll
                for (int f = 0; f < kFrames; f += 4) {
                    const i4 q = {v[f], v[f + 1], v[f + 2], v[f + 3]};
                    *reinterpret_cast<i4 *>(row + t0 + f) = q;
                }
            } else {
#pragma unroll
                for (int f = 0; f < kFrames; ++f)
                    if (t0 + f < a.out_stride) row[t0 + f] = v[f];
            }
        }
    }
    if (costs && mine) costs[lane] = (float)(-cost);
    // frames past the last chunk: blank
    const int64_t t_end = ((int64_t)T + kFrames - 1) / kFrames * kFrames;
    for (int kk = 0; kk < nk; ++kk)
        for (int64_t t = t_end + lane; t < a.out_stride; t += 64) rows[kk * a.out_stride + t] = p.blank;
}

}  // namespace

hipError_t launch_sample(const DevProblem &p, const SampleArgs &a, hipStream_t stream) {
    const int64_t blocks = (int64_t)p.B * ((a.num_samples + 63) / 64);
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    sample_kernel<<<(unsigned)blocks, 64, 0, stream>>>(p, a);
    return hipGetLastError();
}

}  // namespace mrnnt
