// mrnnt_grad.h -- the dense logit-gradient streamers and their launch ladder, over a compile-time row policy P: the
// loss gradient (LossRows, mrnnt_grad.hip), the path-score gradient (PathRows, mrnnt_path.hip), the expected-cost
// gradient (ExpectRows, mrnnt_expect.hip), the factorised-blank loss gradient (HatRows, mrnnt_hat.hip) and the
// factorised-blank twins of the path-score and expected-cost gradients (HatPathRows, HatExpectRows). P supplies
//   Col, column()   what a lattice column sets up once: its band of rows with a gradient; zero(): the other rows' value
//   Slot, stage()   a row's coefficients as they are staged in LDS, two buffers of 256 slots (a dead slot: the row is
//                   stored as zero()), live(); skip() / skipped(): a dead slot whose row already holds zero() (row state)
//   Coef, coef()    a live slot's coefficients as the formula takes them; row(): the same without staging (false:
//                   not live), for the scalar kernel
//   grad_vec(), grad()   the per-vector formula and its scalar twin
//   launch_u()      which kernel a (U, NTL) pair takes;  kNtLoads: whether NTL is ever true
// Everything else -- column walk, segments, barrier, load / store blocks, failed device lengths -- is here once.
#pragma once

#include "mrnnt_device.h"

namespace mrnnt {

constexpr int kGradSeg = 256;  // rows per work unit of the staged kernel: one per thread in phase A
constexpr int kDeadRow = -2;   // label word of a staged row whose gradient is exactly zero (out of band or dead)
constexpr int kSkipRow = -3;   // ... and whose row of grads already holds that zero (p.row_state): not stored again

// Row state (DevProblem::row_state, mrnnt_backward_tracked): the code of a row filled with the value z.
__device__ __forceinline__ unsigned char zero_code(float z) {
    const unsigned bits = __float_as_uint(z);
    return bits == 0u ? 1 : (bits == 0x80000000u ? 2 : 0);  // +0, -0 (either survives the conversion to bf16 / f16)
}

// Staged-coefficient kernel (grad_variant 5, the default, and 6: 2 rows per wave). Work unit = a segment of up to 256
// rows of one lattice column. Phase A: one row per thread, the row's coefficients (P::stage; the loss's row_coef reads
// alpha/beta/den/lp as coalesced vectors along s, the two fp64 exps lane-parallel) go to an LDS slot.
// Phase B: the waves stream the segment's rows; a row's acts loads wait only for one broadcast LDS read, not for
// a chain of dependent scalar loads and fp64 math, so every wave keeps its row(s) of acts in flight. Two LDS
// buffers alternate between work units: one barrier per unit.
// With p.row_state, phase A also keeps the row's state byte (every row is staged by exactly one thread of the grid):
// a dead row whose byte already says "all zero(), same sign" is marked kSkipRow and phase B neither loads nor stores it.
template <class IO, int U, int R, bool NTL, bool NTS, class P>
__global__ __launch_bounds__(256) void grad_staged_kernel(DevProblem p, const float *__restrict__ scale,
                                                          void *__restrict__ grads) {
    if (!resolve_dyn(p)) {  // device-resident lengths failed validation: NaN gradients
        fill_failed_grads<IO>(p, grads);
        return;
    }
    typedef typename IO::V Vec;
    typedef typename P::Slot Slot;
    constexpr int SEG = kGradSeg;
    __shared__ Slot coef[2][SEG];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int VL = p.V / IO::E;
    const int blank = p.blank;
    const Vec *__restrict__ av = reinterpret_cast<const Vec *>(p.acts);
    Vec *__restrict__ gv = reinterpret_cast<Vec *>(grads);

    Cursor cur;
    cur.b = blockIdx.x < p.num_cols ? p.col_b[blockIdx.x] : 0;
    int buf = 0;
    for (int64_t ci = blockIdx.x; ci < p.num_cols; ci += gridDim.x) {
        const int64_t c = visit_col(p, ci);
        if (p.col_mul) cur.b = p.col_b[c];
        else cur.advance(p.col_off, c);
        const int b = cur.b;
        const int T = p.T[b], S = p.S[b];
        const int t = (int)(c - p.col_off[b]);
        const int64_t rowc = p.row_off[b] + (int64_t)t * (S + 1);
        const int64_t arow = acts_col_base(p, b, t, rowc);
        const typename P::Col col = P::column(p, b, c, t, T, S);
        const float sc = scale ? scale[b * p.scale_stride] : 1.0f;  // upstream gradient of the utterance
        const float zf = P::zero(col, sc);
        const Vec zv = splat<IO>(zf);
        const int *__restrict__ lab_b = p.labels + (int64_t)b * p.label_stride;

        for (int seg = 0; seg <= S; seg += SEG, buf ^= 1) {
            {  // phase A
                const int s = seg + tid;
                Slot cf = P::stage(p, col, t, S, s, rowc, lab_b);
                if (p.row_state && s <= S) {
                    unsigned char *st = p.row_state + (arow + s);
                    const unsigned char code = P::live(cf) ? 0 : zero_code(zf);
                    const unsigned char was = *st;
                    if (code && was == code) P::skip(cf);
                    if (was != code) *st = code;
                }
                if (s <= S) coef[buf][tid] = cf;
            }
            __syncthreads();
            const int n = min(SEG, S + 1 - seg);
            for (int i = wave * R; i < n; i += 4 * R) {
                Slot cf[R];
                bool live[R], ok[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    ok[r] = i + r < n;
                    cf[r] = coef[buf][ok[r] ? i + r : i];
                    ok[r] = ok[r] && !P::skipped(cf[r]);
                    live[r] = ok[r] && P::live(cf[r]);
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
                        decltype(auto) rc = P::coef(cf[r]);  // (a value or a reference to the slot, as P has it)
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const int j = base + lane + 64 * u;
                            if (j >= VL) continue;
                            const Vec g = live[r] ? P::template grad_vec<IO>(x[r][u], rc, j, blank, sc) : zv;
                            vstore<NTS>(&gv[(arow + seg + i + r) * (int64_t)VL + j], g);
                        }
                    }
                }
            }
        }
    }
}

// Scalar path (any V, any alignment): one row per wave, lanes stride over v.
template <class IO, class P>
__global__ __launch_bounds__(256) void grad_scalar_kernel(DevProblem p, const float *__restrict__ scale,
                                                          void *__restrict__ grads) {
    if (!resolve_dyn(p)) {  // device-resident lengths failed validation: NaN gradients
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
    Cursor cur;
    cur.b = blockIdx.x < p.num_cols ? p.col_b[blockIdx.x] : 0;
    for (int64_t c = blockIdx.x; c < p.num_cols; c += gridDim.x) {
        cur.advance(p.col_off, c);
        const int b = cur.b;
        const int T = p.T[b], S = p.S[b];
        const int t = (int)(c - p.col_off[b]);
        const int64_t rowc = p.row_off[b] + (int64_t)t * (S + 1);
        const int64_t arow = acts_col_base(p, b, t, rowc);
        const typename P::Col col = P::column(p, b, c, t, T, S);
        const float sc = scale ? scale[b * p.scale_stride] : 1.0f;
        const Sc zs = IO::from_f(P::zero(col, sc));
        const int *__restrict__ lab_b = p.labels + (int64_t)b * p.label_stride;
        for (int s = wave; s <= S; s += 4) {
            Sc *__restrict__ g = gs + (arow + s) * (int64_t)V;
            typename P::Coef rc;
            if (!P::row(p, col, t, S, s, rowc, lab_b, rc)) {
                for (int v = lane; v < V; v += 64) g[v] = zs;
                continue;
            }
            const Sc *__restrict__ z = acts + (arow + s) * (int64_t)V;
            for (int v = lane; v < V; v += 64) g[v] = IO::from_f(P::grad(IO::to_f(z[v]), v, rc, blank, sc));
        }
    }
}

// The slot and the formula of the policies whose rows carry two signed arc weights Wb / We in place of the loss's
// occupancy and posteriors (PathRows, mrnnt_path.hip; ExpectRows, mrnnt_expect.hip):
//   g[v] = (Wb + We) softmax(z_r)[v] - [v == blank] Wb - [v == label(s)] We;  no upstream scale (it is in the weights).
// The policy adds Col / column() / zero() / stage() / row() / launch_u().
struct WeightRows {
    struct Slot {
        float c2;    // den * log2(e)
        float wocc;  // Wb + We (signed; 0 on cancellation)
        float cb;    // Wb
        float ce;    // We
        int lab;     // label(s), -1 for s == S / label == blank / out of range; kDeadRow: the row is stored as zeros
    };
    typedef Slot Coef;
    static __device__ __forceinline__ bool live(const Slot &c) { return c.lab > kDeadRow; }
    static __device__ __forceinline__ void skip(Slot &c) { c.lab = kSkipRow; }
    static __device__ __forceinline__ bool skipped(const Slot &c) { return c.lab == kSkipRow; }
    static __device__ __forceinline__ const Coef &coef(const Slot &c) { return c; }
    // label(s) as the slot holds it
    static __device__ __forceinline__ int slot_label(const DevProblem &p, int S, int s, const int *lab_b) {
        const int lab = (s < S) ? lab_b[s] : -1;
        return (lab == p.blank || (unsigned)lab >= (unsigned)p.V) ? -1 : lab;
    }

    template <class IO>
    static __device__ __forceinline__ typename IO::V grad_vec(const typename IO::V &xv, const Slot &rc, int j, int blank,
                                                              float) {
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
    static __device__ __forceinline__ float grad(float z, int v, const Slot &rc, int blank, float) {
        float g = rc.wocc * fast_exp2(fmaf(z, kLog2e, rc.c2));
        if (v == blank) g -= rc.cb;
        else if (v == rc.lab) g -= rc.ce;
        return g;
    }
};

// The same two signed arc weights over a factorised-blank row (after a forward with p.hat: den = den' = -LSE over the
// non-blank logits, lp.b = log sigmoid(z_blank)) -- HatPathRows, mrnnt_path.hip; HatExpectRows, mrnnt_expect.hip:
//   g[blank]      = We sigmoid(z_b) - Wb sigmoid(-z_b)
//   g[v != blank] = We (exp(z_v + den') - [v == label(s)])
// HatRows' formula (mrnnt_hat.hip) with the posteriors replaced by the weights. We is signed and may be exactly 0 while
// Wb is not, so it cannot go into the exponent as log We: the slot carries the multiplier itself, still one float4.
// The blank element is a select on the row's gb, never arithmetic on exp(z_b + den'), which overflows once the blank
// dominates the row (0 * inf). The policy adds Col / column() / zero() / stage() / row() / launch_u().
struct HatWeightRows {
    typedef float4 Slot;  // {c2, We, gb, label | kDeadRow | kSkipRow}
    struct Coef {
        float c2;  // den' * log2(e); -inf where den' = +inf (every label masked: the non-blank elements are exact zeros)
        float we;  // We
        float gb;  // the blank element
        int lab;   // label(s), -1 for s == S / label == blank / out of range
    };
    static __device__ __forceinline__ Slot dead() { return make_float4(0.0f, 0.0f, 0.0f, __int_as_float(kDeadRow)); }
    static __device__ __forceinline__ bool live(const Slot &cf) { return __float_as_int(cf.w) > kDeadRow; }
    static __device__ __forceinline__ void skip(Slot &cf) { cf.w = __int_as_float(kSkipRow); }
    static __device__ __forceinline__ bool skipped(const Slot &cf) { return __float_as_int(cf.w) == kSkipRow; }
    static __device__ __forceinline__ Coef coef(const Slot &cf) {
        return Coef{cf.x, cf.y, cf.z, __float_as_int(cf.w)};
    }

    // The slot of a live row from its fp64 weights. gb as hat_coef (mrnnt_hat.h) forms it, once per row from
    // lpb = lp[row].b: sigmoid(z_b) = exp(lpb), sigmoid(-z_b) = -expm1(lpb) near 0 and 1 - exp(lpb) elsewhere, each
    // by itself (never (Wb + We) sigmoid(z_b) - Wb); the two products in fp64 from the fp64 weights, one rounding.
    static __device__ __forceinline__ Slot weight_slot(const DevProblem &p, int S, int s, int64_t row, double wb,
                                                       double we, const int *lab_b) {
        const float den = p.den[row];
        const float q = (float)p.lp[row].b;
        const float sp = fast_exp2(q * kLog2e);
        const float sn = q > -0.5f ? -expm1f(q) : 1.0f - sp;
        const float gb = (float)(we * (double)sp - wb * (double)sn);
        const bool masked = den == -NEG_INF_F;  // no label arc: only gb survives
        float c2 = masked ? NEG_INF_F : den * kLog2e;
        if (q != q) c2 = q;  // a NaN (or +inf) blank logit: the whole row is NaN, as its lp pair is
        const int lab = masked ? -1 : WeightRows::slot_label(p, S, s, lab_b);
        return make_float4(c2, (float)we, gb, __int_as_float(lab));
    }

    template <class IO>
    static __device__ __forceinline__ typename IO::V grad_vec(const typename IO::V &xv, const Coef &rc, int j, int blank,
                                                              float) {
        constexpr int E = IO::E;
        float x[E];
        IO::unpack(xv, x);
        const int v0 = j * E;
        const int db = blank - v0;
        const int de = rc.lab >= 0 ? rc.lab - v0 : -1;
#pragma unroll
        for (int i = 0; i < E; ++i) {
            float g = rc.we * fast_exp2(fmaf(x[i], kLog2e, rc.c2));
            g -= de == i ? rc.we : 0.0f;
            x[i] = db == i ? rc.gb : g;
        }
        return IO::pack(x);
    }
    static __device__ __forceinline__ float grad(float z, int v, const Coef &rc, int blank, float) {
        float g = rc.we * fast_exp2(fmaf(z, kLog2e, rc.c2));
        if (v == blank) g = rc.gb;
        else if (v == rc.lab) g -= rc.we;
        return g;
    }
};

// A launch of a kernel that does not keep the row state (every kernel but the staged one): the covered rows become
// "unknown" before it runs, in stream order. (A failed memset is reported by the launch's hipGetLastError.)
static inline void forget_row_state(const DevProblem &p, hipStream_t stream) {
    if (p.row_state && grads_rows(p) > 0) (void)hipMemsetAsync(p.row_state, 0, (size_t)grads_rows(p), stream);
}

template <class IO>
static bool vec_ok(const DevProblem &p, const void *grads) {
    return (p.V % IO::E) == 0 && (reinterpret_cast<uintptr_t>(p.acts) % 16) == 0 &&
           (reinterpret_cast<uintptr_t>(grads) % 16) == 0;
}

// rows per wave of the staged kernel for U vectors per lane: >= 4 KiB of acts in flight per wave
constexpr int staged_rows(int U) { return U == 4 ? 1 : (U == 2 ? 2 : 4); }

// U = 16-byte vectors per lane per chunk: 4 KiB chunks for rows of >= 192 vectors, 2 KiB for >= 96, else 1 KiB
template <class P, class IO, bool NTL, bool NTS>
static void launch_vec(const DevProblem &p, const float *scale, void *grads, int grid, hipStream_t stream) {
    const int VL = p.V / IO::E;
    if (VL >= 192) P::template launch_u<IO, NTL, NTS, 4>(p, scale, grads, grid, stream);
    else if (VL >= 96) P::template launch_u<IO, NTL, NTS, 2>(p, scale, grads, grid, stream);
    else P::template launch_u<IO, NTL, NTS, 1>(p, scale, grads, grid, stream);
}

template <class P, class IO>
static void launch_io(const DevProblem &p, const float *scale, void *grads, int grid, hipStream_t stream) {
    if (!vec_ok<IO>(p, grads)) {
        forget_row_state(p, stream);
        grad_scalar_kernel<IO, P><<<grid, 256, 0, stream>>>(p, scale, grads);
        return;
    }
    const bool nts = tuning().nt_store != 0;
    if constexpr (P::kNtLoads) {  // the policy's acts loads go nontemporal by size (nt_acts_loads)
        if (nt_acts_loads(p, sizeof(typename IO::S))) {
            if (nts) launch_vec<P, IO, true, true>(p, scale, grads, grid, stream);
            else launch_vec<P, IO, true, false>(p, scale, grads, grid, stream);
            return;
        }
    }
    if (nts) launch_vec<P, IO, false, true>(p, scale, grads, grid, stream);
    else launch_vec<P, IO, false, false>(p, scale, grads, grid, stream);
}

template <class P>
static hipError_t launch_grad_rows(const DevProblem &p, int elem, const float *scale, void *grads, int grid,
                                   hipStream_t stream) {
    switch (elem) {
        case ELEM_F32: launch_io<P, IoF32>(p, scale, grads, grid, stream); break;
        case ELEM_BF16: launch_io<P, IoBF16>(p, scale, grads, grid, stream); break;
        case ELEM_F16: launch_io<P, IoF16>(p, scale, grads, grid, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace mrnnt
