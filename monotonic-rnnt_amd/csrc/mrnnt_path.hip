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
//   grad                                the staged gradient kernel of mrnnt_grad.hip with the coefficient phase reading
//                                       Wb / We / den; "in band" = in the hull, "live" = Wb != 0 || We != 0
//
// The hull in the band arrays. The log-softmax reduces, in column c = (b, t), the rows
//   [min(min_s[c] - 1, min_s[c-1]), max(max_s[c], max_s[c-1])]        (align_window, mrnnt_device.h; t = 0: with 0)
// With a(t) / z(t) the lowest / highest visited row of frame t, min_s[c] = a(t) + 1 and max_s[c] = z(t) make that
// window exactly [a(t), z(t)]: a and z are non-decreasing and grow by at most 1 per frame. A column no valid path
// visits (its utterance has none) holds {kHullEmpty, -1}: no rows -- except that align_window always keeps row 0 of
// frame 0, so such an utterance has that one row reduced; nothing reads the result.
#include <algorithm>

#include "mrnnt_device.h"

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

struct PathCoef {
    float c2;    // den * log2(e)
    float wocc;  // Wb + We (signed; 0 on cancellation)
    float cb;    // Wb
    float ce;    // We
    int lab;     // label(s), -1 for s == S / label == blank / out of range; kDead: the row is stored as zeros
};
constexpr int kDead = -2;

__device__ __forceinline__ PathCoef path_coef(const DevProblem &p, int S, int s, int64_t row,
                                              const int *__restrict__ lab_b) {
    PathCoef c{0.0f, 0.0f, 0.0f, 0.0f, kDead};
    const double wb = p.alpha[row], we = p.beta[row];
    if (!(wb != 0.0 || we != 0.0)) return c;
    c.c2 = p.den[row] * kLog2e;
    c.wocc = (float)(wb + we);
    c.cb = (float)wb;
    c.ce = (float)we;
    const int lab = (s < S) ? lab_b[s] : -1;
    c.lab = (lab == p.blank || (unsigned)lab >= (unsigned)p.V) ? -1 : lab;
    return c;
}

template <class IO>
__device__ __forceinline__ typename IO::V path_grad_vec(const typename IO::V &xv, const PathCoef &rc, int j, int blank) {
    constexpr int E = IO::E;
    float x[E];
    IO::unpack(xv, x);
    const int v0 = j * E;
    const int db = blank - v0;
    const int de = rc.lab >= 0 ? rc.lab - v0 : -1;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const float g = rc.wocc * fast_exp2(fmaf(x[i], kLog2e, rc.c2));
        x[i] = g - ((db == i ? rc.cb : 0.0f) + (de == i ? rc.ce : 0.0f));
    }
    return IO::pack(x);
}

// The staged-coefficient kernel of mrnnt_grad.hip (work unit: a segment of up to 256 rows of one lattice column; phase
// A one row per thread into an LDS slot, phase B the waves stream the rows), with phase A reading Wb / We / den.
template <class IO, int U, int R, bool NTL, bool NTS>
__global__ __launch_bounds__(256) void path_grad_staged_kernel(DevProblem p, void *__restrict__ grads) {
    if (!resolve_dyn(p)) {  // device-resident lengths failed validation: NaN gradients
        fill_failed_grads<IO>(p, grads);
        return;
    }
    typedef typename IO::V Vec;
    constexpr int SEG = 256;
    __shared__ float4 coef[2][SEG];
    __shared__ int clab[2][SEG];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int VL = p.V / IO::E;
    const int blank = p.blank;
    const Vec *__restrict__ av = reinterpret_cast<const Vec *>(p.acts);
    Vec *__restrict__ gv = reinterpret_cast<Vec *>(grads);
    const Vec zv = splat<IO>(0.0f);

    Cursor cur;
    cur.b = blockIdx.x < p.num_cols ? p.col_b[blockIdx.x] : 0;
    int buf = 0;
    for (int64_t ci = blockIdx.x; ci < p.num_cols; ci += gridDim.x) {
        const int64_t c = visit_col(p, ci);
        if (p.col_mul) cur.b = p.col_b[c];
        else cur.advance(p.col_off, c);
        const int b = cur.b;
        const int S = p.S[b];
        const int t = (int)(c - p.col_off[b]);
        const int64_t rowc = p.row_off[b] + (int64_t)t * (S + 1);
        const int64_t arow = acts_col_base(p, b, t, rowc);
        const int lo = p.min_s[c] - 1, hi = min(p.max_s[c], S);
        const int *__restrict__ lab_b = p.labels + (int64_t)b * p.label_stride;

        for (int seg = 0; seg <= S; seg += SEG, buf ^= 1) {
            {  // phase A
                const int s = seg + tid;
                PathCoef cf{0.0f, 0.0f, 0.0f, 0.0f, kDead};
                if (s >= lo && s <= hi) cf = path_coef(p, S, s, rowc + s, lab_b);
                if (s <= S) {
                    coef[buf][tid] = make_float4(cf.c2, cf.wocc, cf.cb, cf.ce);
                    clab[buf][tid] = cf.lab;
                }
            }
            __syncthreads();
            const int n = min(SEG, S + 1 - seg);
            for (int i = wave * R; i < n; i += 4 * R) {
                PathCoef rc[R];
                bool live[R], ok[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    ok[r] = i + r < n;
                    const int at = ok[r] ? i + r : i;
                    const float4 f = coef[buf][at];
                    rc[r] = PathCoef{f.x, f.y, f.z, f.w, clab[buf][at]};
                    live[r] = ok[r] && rc[r].lab != kDead;
                }
                for (int base = 0; base < VL; base += 64 * U) {
                    Vec x[R][U];
#pragma unroll
                    for (int r = 0; r < R; ++r)
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const int j = base + lane + 64 * u;
                            if (live[r] && j < VL)
                                x[r][u] = vload<NTL>(&av[(arow + seg + i + r) * (int64_t)VL + j]);
                        }
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (!ok[r]) continue;
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const int j = base + lane + 64 * u;
                            if (j >= VL) continue;
                            const Vec g = live[r] ? path_grad_vec<IO>(x[r][u], rc[r], j, blank) : zv;
                            vstore<NTS>(&gv[(arow + seg + i + r) * (int64_t)VL + j], g);
                        }
                    }
                }
            }
        }
    }
}

// Scalar path (any V, any alignment): one row per wave, lanes stride over v.
template <class IO>
__global__ __launch_bounds__(256) void path_grad_scalar_kernel(DevProblem p, void *__restrict__ grads) {
    if (!resolve_dyn(p)) {
        fill_failed_grads<IO>(p, grads);
        return;
    }
    typedef typename IO::S Sc;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int V = p.V;
    const int blank = p.blank;
    const Sc *__restrict__ acts = reinterpret_cast<const Sc *>(p.acts);
    Sc *__restrict__ gs = reinterpret_cast<Sc *>(grads);
    const Sc zs = IO::from_f(0.0f);
    Cursor cur;
    cur.b = blockIdx.x < p.num_cols ? p.col_b[blockIdx.x] : 0;
    for (int64_t c = blockIdx.x; c < p.num_cols; c += gridDim.x) {
        cur.advance(p.col_off, c);
        const int b = cur.b;
        const int S = p.S[b];
        const int t = (int)(c - p.col_off[b]);
        const int64_t rowc = p.row_off[b] + (int64_t)t * (S + 1);
        const int64_t arow = acts_col_base(p, b, t, rowc);
        const int lo = p.min_s[c] - 1, hi = min(p.max_s[c], S);
        const int *__restrict__ lab_b = p.labels + (int64_t)b * p.label_stride;
        for (int s = wave; s <= S; s += 4) {
            Sc *__restrict__ g = gs + (arow + s) * (int64_t)V;
            PathCoef rc{0.0f, 0.0f, 0.0f, 0.0f, kDead};
            if (s >= lo && s <= hi) rc = path_coef(p, S, s, rowc + s, lab_b);
            if (rc.lab == kDead) {
                for (int v = lane; v < V; v += 64) g[v] = zs;
                continue;
            }
            const Sc *__restrict__ z = acts + (arow + s) * (int64_t)V;
            for (int v = lane; v < V; v += 64) {
                float gvv = rc.wocc * fast_exp2(fmaf(IO::to_f(z[v]), kLog2e, rc.c2));
                if (v == blank) gvv -= rc.cb;
                else if (v == rc.lab) gvv -= rc.ce;
                g[v] = IO::from_f(gvv);
            }
        }
    }
}

template <class IO, bool NTL, bool NTS>
void launch_path_vec(const DevProblem &p, void *grads, int grid, hipStream_t stream) {
    // 16-byte vectors per lane per chunk and rows per wave as the loss's staged kernel takes them (mrnnt_grad.hip)
    const int VL = p.V / IO::E;
    if (VL >= 192) path_grad_staged_kernel<IO, 4, 1, NTL, NTS><<<grid, 256, 0, stream>>>(p, grads);
    else if (VL >= 96) path_grad_staged_kernel<IO, 2, 2, NTL, NTS><<<grid, 256, 0, stream>>>(p, grads);
    else path_grad_staged_kernel<IO, 1, 4, NTL, NTS><<<grid, 256, 0, stream>>>(p, grads);
}

template <class IO>
void launch_path_io(const DevProblem &p, void *grads, int grid, hipStream_t stream) {
    const bool vec = (p.V % IO::E) == 0 && (reinterpret_cast<uintptr_t>(p.acts) % 16) == 0 &&
                     (reinterpret_cast<uintptr_t>(grads) % 16) == 0;
    if (!vec) {
        path_grad_scalar_kernel<IO><<<grid, 256, 0, stream>>>(p, grads);
        return;
    }
    // few rows are read (at most B K T of them): the loads keep the default policy; the stores are the pass
    if (tuning().nt_store != 0) launch_path_vec<IO, false, true>(p, grads, grid, stream);
    else launch_path_vec<IO, false, false>(p, grads, grid, stream);
}

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
    switch (elem) {
        case ELEM_F32: launch_path_io<IoF32>(p, grads, grid, stream); break;
        case ELEM_BF16: launch_path_io<IoBF16>(p, grads, grid, stream); break;
        case ELEM_F16: launch_path_io<IoF16>(p, grads, grid, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace mrnnt
