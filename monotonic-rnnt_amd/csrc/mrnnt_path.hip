// mrnnt_path.hip -- differentiable scores of given alignments (mrnnt_path_forward / mrnnt_path_backward,
// include/mrnnt.h): for K alignment rows per utterance, path_costs[b, k] = -sum_t lp(arc_t) along the walk of row
// (b, k), and the logit gradient of sum_k w[b, k] * path_costs[b, k],
//   g[r, v] = Wocc(r) softmax(z_r)[v] - [v == blank] Wb(r) - [v == label(s)] We(r),
// Wb / We the weights of the valid paths that leave row r by its blank / label arc. One forward and one dense
// gradient pass whatever K is.
//
// A walk is a prefix count: s_k(t) = the non-blank entries among frames < t. Lanes are frames; a 64-frame block's
// positions are a ballot and a popcount on top of the block's carry s_k(64 * blk), which the walk kernel stores per
// (block, k) so that the kernels that own (utterance, frame block) need no scan of their own.
//   walk  (one wave per path)           validity, block carries
//   hull  (one wave per frame block)    [min_k s_k(t), max_k s_k(t)] over the valid paths, written into the plan's band
//                                       arrays in the form the log-softmax's alignment window reads (below)
//   log-softmax over the hull           launch_softmax, unchanged: den and lp of the hull rows, no other acts row
//   score (one wave per path)           gather of lp along the walk, fp64, fixed order
//   coef  (one wave per frame block)    Wb / We (the workspace's alpha / beta arrays) zeroed over the hull, then
//                                       w[b, k] added in ascending k, lane = frame: a lane's rows are its own column's,
//                                       so no atomics and a fixed order
//   grad                                the gradient streamers of mrnnt_grad.h over PathRows: coefficients from Wb /
//                                       We / den; "in band" = in the hull, "live" = Wb != 0 || We != 0
// The factorised blank (mrnnt_hat_path_*): the same walk, hull, score and coef kernels -- they read lp / alpha / beta /
// the band arrays, never a logit -- around the HAT flavour of the log-softmax (p.hat) and the gradient over
// HatPathRows, g[blank] = We sigmoid(z_b) - Wb sigmoid(-z_b), g[v != blank] = We (exp(z_v + den') - [v == label(s)]).
//
// The hull in the band arrays. The log-softmax reduces, in column c = (b, t), the rows
//   [min(min_s[c] - 1, min_s[c-1]), max(max_s[c], max_s[c-1])]        (align_window, mrnnt_device.h; t = 0: with 0)
// With a(t) / z(t) the lowest / highest visited row of frame t, min_s[c] = a(t) + 1 and max_s[c] = z(t) make that
// window exactly [a(t), z(t)]: a and z are non-decreasing and grow by at most 1 per frame. A column no valid path
// visits (its utterance has none) holds {kHullEmpty, -1}: no rows -- except that align_window always keeps row 0 of
// frame 0, so such an utterance has that one row reduced; nothing reads the result.
#include <algorithm>

#include "mrnnt_grad.h"

namespace mrnnt {

namespace {

constexpr int kHullEmpty = 1 << 29;

__device__ __forceinline__ bool lengths_failed(const DevProblem &p) {
    return p.dyn && __builtin_amdgcn_readfirstlane(p.dyn->status);
}

// first carry slot of utterance b: its 64-frame blocks follow one another, every utterance starting a slot of its own
__device__ __forceinline__ int64_t block_base(const DevProblem &p, int b) { return (p.col_off[b] >> 6) + b; }

// One 64-frame block of alignment row `row` at frame t (in: t < T): the lane's position given the block's carry, and
// whether its frame emits a label. n: the labels the block emits (uniform).
struct BlockWalk {
    int v, pos, n;
    bool label;
};

__device__ __forceinline__ BlockWalk block_walk(const int *__restrict__ row, int t, bool in, int blank, int carry) {
    const int lane = threadIdx.x & 63;
    BlockWalk w;
    w.v = in ? row[t] : blank;
    w.label = in && w.v != blank;
    const unsigned long long m = __ballot(w.label);
    w.pos = carry + __popcll(m & ((1ull << lane) - 1ull));
    w.n = __popcll(m);
    return w;
}

// walk: one wave per (b, k). valid[b, k], and the carry of every block up to the first bad entry.
__global__ __launch_bounds__(64) void path_walk_kernel(DevProblem p, PathArgs a) {
    if (lengths_failed(p)) return;  // the lengths may be anything: nothing is touched (the score kernel reports)
    const int b = (int)(blockIdx.x / (unsigned)a.K), k = (int)(blockIdx.x - (unsigned)b * a.K);
    const int lane = threadIdx.x;
    const int T = p.T[b], S = p.S[b];
    const int *__restrict__ row = a.al + ((int64_t)b * a.K + k) * a.stride;
    const int *__restrict__ lab = p.labels + (int64_t)b * p.label_stride;
    int *__restrict__ carry = a.carry + block_base(p, b) * a.K + k;
    int s = 0;
    bool ok = true;
    for (int t0 = 0; t0 < T; t0 += 64) {
        if (lane == 0) carry[(int64_t)(t0 >> 6) * a.K] = s;
        const BlockWalk w = block_walk(row, t0 + lane, t0 + lane < T, p.blank, s);
        // a label entry must be labels[b, s] of the position it is met at, s < S_b; negative values are never labels
        const bool bad = w.label && (w.v < 0 || w.pos >= S || lab[w.pos] != w.v);
        if (__ballot(bad)) {
            ok = false;
            break;
        }
        s += w.n;
    }
    if (lane == 0) a.valid[(int64_t)b * a.K + k] = (ok && s == S) ? 1 : 0;
}

// hull: one wave per (b, 64-frame block), grid (x, B), the waves of x striding over the blocks.
__global__ __launch_bounds__(256) void path_hull_kernel(DevProblem p, PathArgs a) {
    if (lengths_failed(p)) return;
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int T = p.T[b];
    const int64_t c0 = p.col_off[b];
    const int64_t base = block_base(p, b);
    for (int blk = blockIdx.x * 4 + wave; blk * 64 < T; blk += gridDim.x * 4) {
        const int t = blk * 64 + lane;
        const bool in = t < T;
        int lo = kHullEmpty - 1, hi = -1;
        for (int k = 0; k < a.K; ++k) {
            if (!a.valid[(int64_t)b * a.K + k]) continue;  // (uniform)
            const int *__restrict__ row = a.al + ((int64_t)b * a.K + k) * a.stride;
            const BlockWalk w = block_walk(row, t, in, p.blank, a.carry[(base + blk) * a.K + k]);
            lo = min(lo, w.pos);
            hi = max(hi, w.pos);
        }
        if (in) {
            a.min_s[c0 + t] = lo + 1;
            a.max_s[c0 + t] = hi;
        }
    }
}

// score: one wave per (b, k); lane partial sums over the blocks, then a butterfly: a fixed order.
__global__ __launch_bounds__(64) void path_score_kernel(DevProblem p, PathArgs a) {
    const int b = (int)(blockIdx.x / (unsigned)a.K), k = (int)(blockIdx.x - (unsigned)b * a.K);
    const int lane = threadIdx.x;
    float *out = a.costs + (int64_t)b * a.K + k;
    if (lengths_failed(p)) {
        if (lane == 0) *out = __builtin_nanf("");
        return;
    }
    if (!a.valid[(int64_t)b * a.K + k]) {
        if (lane == 0) *out = __builtin_huge_valf();
        return;
    }
    const int T = p.T[b], W = p.S[b] + 1;
    const int *__restrict__ row = a.al + ((int64_t)b * a.K + k) * a.stride;
    const int64_t r0 = p.row_off[b];
    int s = 0;
    double acc = 0.0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool in = t < T;
        const BlockWalk w = block_walk(row, t, in, p.blank, s);
        if (in) {
            const Lp l = p.lp[r0 + (int64_t)t * W + w.pos];
            acc += w.label ? l.e : l.b;
        }
        s += w.n;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) *out = (float)(-acc);
}

// coef: one wave per (b, 64-frame block). Wb = p.alpha, We = p.beta over the hull rows of the block's columns.
__global__ __launch_bounds__(256) void path_coef_kernel(DevProblem p, PathArgs a) {
    if (lengths_failed(p)) return;
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int T = p.T[b], S = p.S[b], W = S + 1;
    const int64_t c0 = p.col_off[b], r0 = p.row_off[b];
    const int64_t base = block_base(p, b);
    for (int blk = blockIdx.x * 4 + wave; blk * 64 < T; blk += gridDim.x * 4) {
        const int t = blk * 64 + lane;
        const bool in = t < T;
        const int64_t rowc = r0 + (int64_t)t * W;
        int lo = 0, hi = -1;
        if (in) {
            lo = max(a.min_s[c0 + t] - 1, 0);
            hi = min(a.max_s[c0 + t], S);
            for (int s = lo; s <= hi; ++s) {
                p.alpha[rowc + s] = 0.0;
                p.beta[rowc + s] = 0.0;
            }
        }
        for (int k = 0; k < a.K; ++k) {
            if (!a.valid[(int64_t)b * a.K + k]) continue;  // (uniform)
            const int *__restrict__ row = a.al + ((int64_t)b * a.K + k) * a.stride;
            const BlockWalk w = block_walk(row, t, in, p.blank, a.carry[(base + blk) * a.K + k]);
            const double wk = a.w ? (double)a.w[(int64_t)b * a.K + k] : 1.0;
            // (inside the hull by construction; the test keeps the stores inside the column's hull rows when the
            // workspace is not that of a forward on these alignments)
            if (in && w.pos >= lo && w.pos <= hi) {
                double *cell = (w.label ? p.beta : p.alpha) + rowc + w.pos;
                *cell += wk;
            }
        }
    }
}

// ---- gradient ------------------------------------------------------------------------------------------------------

// The path scores' rows for the shared streamers (mrnnt_grad.h): band = the hull of the column, a row's staged
// coefficients from Wb / We / den, the other rows plain zeros; no upstream scale (the weights are in Wb / We).
// Slot, formula and scalar twin: WeightRows (mrnnt_grad.h).
struct PathRows : WeightRows {
    struct Col {
        int lo, hi;
    };
    static __device__ __forceinline__ Col column(const DevProblem &p, int, int64_t c, int, int, int S) {
        return Col{p.min_s[c] - 1, min(p.max_s[c], S)};
    }
    static __device__ __forceinline__ float zero(const Col &, float) { return 0.0f; }

    // (as the loss's row_coef: nothing of the row is read before it is known to be in the hull)
    static __device__ __forceinline__ Slot stage(const DevProblem &p, const Col &col, int, int S, int s, int64_t rowc,
                                                 const int *lab_b) {
        Slot c{0.0f, 0.0f, 0.0f, 0.0f, kDeadRow};
        if (!(s >= col.lo && s <= col.hi)) return c;
        const int64_t row = rowc + s;
        const double wb = p.alpha[row], we = p.beta[row];
        if (!(wb != 0.0 || we != 0.0)) return c;
        c.c2 = p.den[row] * kLog2e;
        c.wocc = (float)(wb + we);
        c.cb = (float)wb;
        c.ce = (float)we;
        c.lab = slot_label(p, S, s, lab_b);
        return c;
    }
    static __device__ __forceinline__ bool row(const DevProblem &p, const Col &col, int t, int S, int s, int64_t rowc,
                                               const int *lab_b, Coef &c) {
        c = stage(p, col, t, S, s, rowc, lab_b);
        return live(c);
    }

    // few rows are read (at most B K T of them): the loads keep the default policy; the stores are the pass
    static constexpr bool kNtLoads = false;
    template <class IO, bool NTL, bool NTS, int U>
    static void launch_u(const DevProblem &p, const float *, void *grads, int grid, hipStream_t stream) {
        static_assert(!NTL, "path scores never load nontemporally");
        grad_staged_kernel<IO, U, staged_rows(U), false, NTS, PathRows><<<grid, 256, 0, stream>>>(p, nullptr, grads);
    }
};

// The factorised-blank twin (mrnnt_hat_path_backward, after a forward with p.hat over the hull): PathRows' band, zero
// value and liveness rule (Wb != 0 || We != 0 in fp64: Wb = -We stays live), HatWeightRows' slot and formula.
struct HatPathRows : HatWeightRows {
    typedef PathRows::Col Col;
    static __device__ __forceinline__ Col column(const DevProblem &p, int b, int64_t c, int t, int T, int S) {
        return PathRows::column(p, b, c, t, T, S);
    }
    static __device__ __forceinline__ float zero(const Col &, float) { return 0.0f; }

    static __device__ __forceinline__ Slot stage(const DevProblem &p, const Col &col, int, int S, int s, int64_t rowc,
                                                 const int *lab_b) {
        if (!(s >= col.lo && s <= col.hi)) return dead();
        const int64_t row = rowc + s;
        const double wb = p.alpha[row], we = p.beta[row];
        if (!(wb != 0.0 || we != 0.0)) return dead();
        return weight_slot(p, S, s, row, wb, we, lab_b);
    }
    static __device__ __forceinline__ bool row(const DevProblem &p, const Col &col, int t, int S, int s, int64_t rowc,
                                               const int *lab_b, Coef &c) {
        const Slot cf = stage(p, col, t, S, s, rowc, lab_b);
        c = coef(cf);
        return live(cf);
    }

    static constexpr bool kNtLoads = false;
    template <class IO, bool NTL, bool NTS, int U>
    static void launch_u(const DevProblem &p, const float *, void *grads, int grid, hipStream_t stream) {
        static_assert(!NTL, "path scores never load nontemporally");
        grad_staged_kernel<IO, U, staged_rows(U), false, NTS, HatPathRows><<<grid, 256, 0, stream>>>(p, nullptr, grads);
    }
};

// x workgroups of 4 waves per utterance for the (utterance, frame block) kernels
dim3 block_grid(const DevProblem &p, int T_bound) {
    const int blocks = std::max(1, (T_bound + 63) / 64);
    return dim3((unsigned)std::min(64, (blocks + 3) / 4), (unsigned)p.B, 1);
}

}  // namespace

hipError_t launch_path_walk(const DevProblem &p, const PathArgs &a, int T_bound, hipStream_t stream) {
    const int64_t waves = (int64_t)p.B * a.K;
    if (waves > 0x7fffffff || p.B > 65535) return hipErrorInvalidValue;
    path_walk_kernel<<<(unsigned)waves, 64, 0, stream>>>(p, a);
    path_hull_kernel<<<block_grid(p, T_bound), 256, 0, stream>>>(p, a);
    return hipGetLastError();
}

hipError_t launch_path_score(const DevProblem &p, const PathArgs &a, hipStream_t stream) {
    path_score_kernel<<<(unsigned)((int64_t)p.B * a.K), 64, 0, stream>>>(p, a);
    return hipGetLastError();
}

hipError_t launch_path_coef(const DevProblem &p, const PathArgs &a, int T_bound, hipStream_t stream) {
    if ((int64_t)p.B * a.K > 0x7fffffff || p.B > 65535) return hipErrorInvalidValue;
    path_coef_kernel<<<block_grid(p, T_bound), 256, 0, stream>>>(p, a);
    return hipGetLastError();
}

hipError_t launch_path_grad(const DevProblem &p, int elem, void *grads, int grid, hipStream_t stream) {
    return launch_grad_rows<PathRows>(p, elem, nullptr, grads, grid, stream);
}

hipError_t launch_hat_path_grad(const DevProblem &p, int elem, void *grads, int grid, hipStream_t stream) {
    return launch_grad_rows<HatPathRows>(p, elem, nullptr, grads, grid, stream);
}

}  // namespace mrnnt
