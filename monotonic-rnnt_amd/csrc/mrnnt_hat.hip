// mrnnt_hat.hip -- logit gradient of the factorised-blank (HAT) loss, mrnnt_hat_backward: blank is a Bernoulli on its
// own logit z_b, the labels a softmax over the other V - 1 logits (the forward: the HAT flavour of the log-softmax
// bodies, mrnnt_lsm.h). With the arc posteriors of the row, cb = exp(lpb + alpha(t-1,s) + beta(t+1,s) - ll) and
// ce = exp(lpe + alpha(t-1,s) + beta(t+1,s+1) - ll) (0 at s = S),
//   g[b]      = ce sigmoid(z_b) - cb sigmoid(-z_b)
//   g[v != b] = ce (exp(z_v + den') - [v == label(s)]),   den' = -LSE_{u != b} z_u
// times grad_scale[b]. Per element it is the loss's one fma + one v_exp_f32 (ce is folded into the exponent in fp64)
// and a select; the blank element is formed once per row from lpb = log sigmoid(z_b), each sigmoid by itself
// (sigmoid(-z_b) = -expm1(lpb) near 0), never as (cb + ce) sigmoid(z_b) - cb. The staged and the scalar kernel are the
// shared streamers of mrnnt_grad.h over the row policy HatRows below; rows outside the band and dead rows are stored
// as the loss stores them (zero_row_value), padding rows by launch_pad_zero.
#include "mrnnt_grad.h"
#include "mrnnt_hat.h"  // HatCoef / hat_coef: the row coefficients, shared with the fused joint

namespace mrnnt {

struct HatRows {
    struct Col {
        int T, lo, hi;
        double ll;
    };
    static __device__ __forceinline__ Col column(const DevProblem &p, int b, int64_t, int t, int T, int S) {
        return Col{T, max(0, t - (T - S)), min(t, S), p.ll[b]};
    }
    static __device__ __forceinline__ float zero(const Col &col, float sc) { return zero_row_value(col.ll, sc); }

    typedef HatCoef Coef;
    static __device__ __forceinline__ bool row(const DevProblem &p, const Col &col, int t, int S, int s, int64_t rowc,
                                               const int *lab_b, Coef &rc) {
        return s >= col.lo && s <= col.hi && hat_coef(p, t, col.T, S, s, rowc + s, col.ll, lab_b, rc);
    }

    typedef float4 Slot;  // {c2, ce, gb, label | kDeadRow | kSkipRow}
    static __device__ __forceinline__ Slot stage(const DevProblem &p, const Col &col, int t, int S, int s, int64_t rowc,
                                                 const int *lab_b) {
        Slot cf = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(kDeadRow));
        HatCoef rc;
        if (row(p, col, t, S, s, rowc, lab_b, rc)) cf = make_float4(rc.c2, rc.ce, rc.gb, __int_as_float(rc.lab));
        return cf;
    }
    static __device__ __forceinline__ bool live(const Slot &cf) { return __float_as_int(cf.w) > kDeadRow; }
    static __device__ __forceinline__ void skip(Slot &cf) { cf.w = __int_as_float(kSkipRow); }
    static __device__ __forceinline__ bool skipped(const Slot &cf) { return __float_as_int(cf.w) == kSkipRow; }
    static __device__ __forceinline__ Coef coef(const Slot &cf) {
        return HatCoef{cf.x, cf.y, cf.z, __float_as_int(cf.w)};
    }

    template <class IO>
    static __device__ __forceinline__ typename IO::V grad_vec(const typename IO::V &xv, const HatCoef &rc, int j,
                                                              int blank, float sc) {
        constexpr int E = IO::E;
        float x[E];
        IO::unpack(xv, x);
        const int v0 = j * E;
        const int db = blank - v0;
        const int de = rc.lab >= 0 ? rc.lab - v0 : -1;
#pragma unroll
        for (int i = 0; i < E; ++i) {
            float g = fast_exp2(fmaf(x[i], kLog2e, rc.c2));
            g -= de == i ? rc.ce : 0.0f;
            g = db == i ? rc.gb : g;
            x[i] = g * sc;
        }
        return IO::pack(x);
    }
    static __device__ __forceinline__ float grad(float z, int v, const HatCoef &rc, int blank, float sc) {
        float g = fast_exp2(fmaf(z, kLog2e, rc.c2));
        if (v == blank) g = rc.gb;
        else if (v == rc.lab) g -= rc.ce;
        return g * sc;
    }

    static constexpr bool kNtLoads = true;
    // the staged kernel for every row length: 4 / 2 / 1 rows per wave for U = 1 / 2 / 4
    template <class IO, bool NTL, bool NTS, int U>
    static void launch_u(const DevProblem &p, const float *scale, void *grads, int grid, hipStream_t stream) {
        grad_staged_kernel<IO, U, staged_rows(U), NTL, NTS, HatRows><<<grid, 256, 0, stream>>>(p, scale, grads);
    }
};

hipError_t launch_hat_grad(const DevProblem &p, int elem, const float *scale, void *grads, int grid,
                           hipStream_t stream) {
    return launch_grad_rows<HatRows>(p, elem, scale, grads, grid, stream);
}

}  // namespace mrnnt
