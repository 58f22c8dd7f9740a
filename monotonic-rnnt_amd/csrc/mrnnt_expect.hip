// mrnnt_expect.hip -- expected path costs with a gradient (mrnnt_expect_forward / mrnnt_expect_backward,
// include/mrnnt.h): for a cost that adds up over arcs, f(path) = sum_t cost(arc_t) with wb(t, s) on the blank arc and
// we(t, s) on the label arc of row (t, s),
//   expected[b] = sum_path p(path | labels, acts) f(path)
// and the logit gradient of g_e . expected + g_c . costs in ONE dense pass. The first-order expectation semiring over
// the state the forward keeps: with alpha(t, s) after frame t, beta(t, s) before frame t (mrnnt_posteriors' conventions),
//   A(t, s)  = the mean cost of the path prefixes that end in state (t, s)      A(-1, .) = 0
//   Bk(t, s) = the mean cost of the path suffixes that start in state (t, s)   Bk(T, .) = 0
//   R = expected[b] = A(T-1, S) = Bk(0, 0)
//   cb(t, s) = blank_post (A(t-1, s) + wb(t, s) + Bk(t+1, s)   - R)
//   ce(t, s) = label_post (A(t-1, s) + we(t, s) + Bk(t+1, s+1) - R)
//   d expected / d z[r, v] = cb ([v == blank] - softmax(z_r)[v]) + ce ([v == label(s)] - softmax(z_r)[v]).
//
// The recursion (expect_kernel): one launch after the forward, one workgroup per (utterance, direction) -- A forward in
// time, Bk backward, concurrently -- lanes along s, K cells per lane; the neighbour cell crosses lanes with the DPP wave
// shifts and waves through a double-buffered LDS slot with one barrier per step, as recursion_kernel does. A step mixes
// the two arcs that enter (leave) the cell,
//   new = q (self + cost_x) + p (neighbour + cost_y),   p = e^y / (e^x + e^y),  q = 1 - p,
// x / y the log-weights of the blank / label arc (x = alpha(t-1, s) + lpb(t, s), y = alpha(t-1, s-1) + lpe(t, s-1);
// backward: x = lpb(t, s) + beta(t+1, s), y = lpe(t, s) + beta(t+1, s+1)). p is the logistic of y - x: the smaller of
// the two weights is e / (1 + e), e = exp(-|x - y|), on the fp32 hardware exp2 / rcp (absolute error <= ~1.5e-7) and
// the other one is 1 minus it in fp64, so the pair sums to exactly 1: a convex combination whatever the rounding (a
// constant cost c gives c T_b). The weights do not depend on A: the state, lp and cost values of a step are loaded D
// steps ahead into a register ring, the mix {q, p, c = q cost_x + p cost_y} is formed beside the chain, and the
// dependent chain of a step is the neighbour shift and two fp64 FMAs.
//
// Which cells are read. Cells are masked by the band BOUNDS -- the monotonic band, and min_s / max_s under a
// restricting alignment -- never by alpha = -inf: the lean recursion leaves finite values outside the monotonic band,
// and lp is written only for the rows the forward reduced. The states before frame u (after frame u - 1) are
//   band(0) = {0};   band(u) = [max(u - (T - S), min_s(u-1), 0), min(u, S, max_s(u-1))],
// an arc whose source (target) state lies outside it has weight 0 (a select on the loaded value, no arithmetic), and a
// cell outside band(u), or with both arcs at -inf (masked logits), holds A = 0 (Bk = 0). Every cell of [0, S] is
// written each step, so ExpectRows reads no uninitialised value.
//
// The gradient: the shared streamers of mrnnt_grad.h over ExpectRows, the slot and the formula those of the path
// scores (WeightRows) with
//   Wb = g_c blank_post - g_e cb,   We = g_c label_post - g_e ce     (the deviation A + w + Bk - R first, in fp64).
#include <algorithm>

#include "mrnnt_dp.h"
#include "mrnnt_grad.h"

namespace mrnnt {

namespace {

// band(u): the states before frame u, 0 <= u <= T (uniform)
template <bool BAND>
__device__ __forceinline__ void state_band(const DevProblem &p, int64_t c0, int T, int S, int u, int &lo, int &hi) {
    lo = max(u - (T - S), 0);
    hi = min(u, S);
    if (BAND && u > 0) {
        lo = max(lo, p.min_s[c0 + u - 1]);
        hi = min(hi, p.max_s[c0 + u - 1]);
    }
    if (u == 0) hi = 0;
}

// new = q * self + p * neighbour + c
struct Mix {
    double q, p, c;
};

__device__ __forceinline__ Mix arc_mix(double x, double y, float cx, float cy) {
    const bool ybig = y > x;
    const float e = fast_exp2((float)(-fabs(x - y)) * kLog2e);
    const double wl = (double)(e * __builtin_amdgcn_rcpf(1.0f + e));  // the smaller weight, <= 1/2
    Mix m;
    m.p = ybig ? 1.0 - wl : wl;
    m.q = ybig ? wl : 1.0 - wl;
    if (x == NEG_INF_D && y == NEG_INF_D) m.p = m.q = 0.0;  // no path reaches the cell
    // (a cost on an arc of weight 0 is not multiplied: it may be anything)
    m.c = (m.q != 0.0 ? m.q * (double)cx : 0.0) + (m.p != 0.0 ? m.p * (double)cy : 0.0);
    return m;
}

// One direction of one utterance. FWD: A(t, .) for t = 0 .. T-1 into p.ex_A, then R and expected[b]. BWD: Bk(t, .)
// for t = T-1 .. 0 into p.ex_Bk.
template <int K, int D, int NW, bool BAND, bool BWD>
__device__ __forceinline__ void expect_pass(const DevProblem &p, int b, float *__restrict__ expected,
                                            double (*xb)[8]) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int T = p.T[b], S = p.S[b], W = S + 1;
    const int64_t r0 = p.row_off[b], c0 = p.col_off[b];
    const int s0 = (wave * 64 + lane) * K;
    static_assert(NW == 1 || NW == 2 || NW == 4 || NW == 8, "cross-wave slots sized for <= 8 waves");
    const double *__restrict__ state = BWD ? p.beta : p.alpha;
    double *__restrict__ out = BWD ? p.ex_Bk : p.ex_A;

    // the ring: what step t reads, loaded D steps ahead. xs / ys: the state of the blank / label arc's other end;
    // lb / le: the arcs' log-probabilities; cx / cy: their costs; the bands of the step's own and other states
    double xs[D][K], ys[D][K], lb[D][K], le[D][K];
    float cx[D][K], cy[D][K];
    int lo_c[D], hi_c[D], lo_o[D], hi_o[D];
    auto load = [&](int t, int d) {
        // the other end's frame, clamped into the array (the boundary state is set at the use)
        const int to = BWD ? min(t + 1, T - 1) : max(t - 1, 0);
        const int64_t rs = r0 + (int64_t)to * W, rl = r0 + (int64_t)t * W;
        const int64_t ar = acts_col_base(p, b, t, rl);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int s = min(s0 + k, S);                              // lanes past S are masked by the band
            const int sn = BWD ? min(s + 1, S) : max(s - 1, 0);        // the label arc's other end
            const int se = BWD ? s : sn;                               // ... and its row
            xs[d][k] = state[rs + s];
            ys[d][k] = state[rs + sn];
            lb[d][k] = p.lp[rl + s].b;
            le[d][k] = p.lp[rl + se].e;
            cx[d][k] = p.ex_wb ? p.ex_wb[ar + s] : 0.0f;
            cy[d][k] = p.ex_we ? p.ex_we[ar + se] : 0.0f;
        }
        state_band<BAND>(p, c0, T, S, BWD ? t : t + 1, lo_c[d], hi_c[d]);
        state_band<BAND>(p, c0, T, S, BWD ? t + 1 : t, lo_o[d], hi_o[d]);
    };

    double a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = 0.0;
    const int first = BWD ? T - 1 : 0;
    if (NW > 1 && lane == 0) xb[(first + 1) & 1][wave] = 0.0;  // the cross-wave neighbour of the first step
#pragma unroll
    for (int d = 0; d < D; ++d) load(BWD ? max(T - 1 - d, 0) : min(d, T - 1), d);
    __syncthreads();

    for (int i0 = 0; i0 < T; i0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int i = i0 + d;
            if (i >= T) break;
            const int t = BWD ? T - 1 - i : i;
            const bool edge = t == first;  // the other end is the boundary state: 0 on its one cell
            Mix m[K];
            bool in[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int s = s0 + k;
                const int sn = BWD ? s + 1 : s - 1;
                const bool okx = s >= lo_o[d] && s <= hi_o[d];
                const bool oky = sn >= lo_o[d] && sn <= hi_o[d] && (BWD ? s < S : s > 0);
                const double x = okx ? (edge ? 0.0 : xs[d][k]) + lb[d][k] : NEG_INF_D;
                const double y = oky ? (edge ? 0.0 : ys[d][k]) + le[d][k] : NEG_INF_D;
                m[k] = arc_mix(x, y, cx[d][k], cy[d][k]);
                in[k] = s >= lo_c[d] && s <= hi_c[d];
            }
            // ---- the dependent chain: the neighbour shift and two FMAs per cell
            double carry = BWD ? dpp_shl1(a[0]) : dpp_shr1(a[K - 1]);
            if (NW > 1 && lane == (BWD ? 63 : 0) && wave != (BWD ? NW - 1 : 0))
                carry = xb[(t + 1) & 1][BWD ? wave + 1 : wave - 1];
            double na[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double nb = BWD ? (k == K - 1 ? carry : a[k + 1]) : (k == 0 ? carry : a[k - 1]);
                const double v = fma(m[k].p, nb, fma(m[k].q, a[k], m[k].c));
                na[k] = in[k] ? v : 0.0;
            }
            double *o = out + r0 + (int64_t)t * W + s0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                a[k] = na[k];
                if (s0 + k < W) o[k] = na[k];
            }
            if (NW > 1 && lane == (BWD ? 0 : 63)) xb[t & 1][wave] = na[BWD ? 0 : K - 1];
            load(BWD ? max(t - D, 0) : min(t + D, T - 1), d);
            if (NW > 1) __syncthreads();
        }
    }
    if (!BWD) {
        const double ll = p.ll[b];
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (s0 + k == S) {
                p.ex_R[b] = a[k];
                if (expected) expected[b] = __builtin_isfinite(ll) ? (float)a[k] : __builtin_nanf("");
            }
    }
}

template <int K, int D, int NW, bool BAND>
__global__ __launch_bounds__(64 * NW) void expect_kernel(DevProblem p, int with_bk, float *__restrict__ expected) {
    __shared__ double xb[2][8];
    const int b = with_bk ? (int)(blockIdx.x >> 1) : (int)blockIdx.x;
    const bool bwd = with_bk && (blockIdx.x & 1);
    if (p.dyn && __builtin_amdgcn_readfirstlane(p.dyn->status)) {
        // device-resident lengths that failed validation: the lengths may be anything, no lattice array is touched
        if (!bwd && threadIdx.x == 0) {
            p.ex_R[b] = __builtin_nan("");
            if (expected) expected[b] = __builtin_nanf("");
        }
        return;
    }
    if (bwd)
        expect_pass<K, D, NW, BAND, true>(p, b, expected, xb);
    else
        expect_pass<K, D, NW, BAND, false>(p, b, expected, xb);
}

struct ExpectLaunch {  // launch_by_width's go<K, NW>()
    const DevProblem &p;
    int with_bk;
    float *expected;
    hipStream_t stream;
    template <int K, int NW>
    void go() const {
        // D = steps loaded ahead (register ring), shallower where K cells per lane use the registers
        constexpr int D = K == 1 ? 8 : (K == 2 ? 4 : 2);
        const int blocks = with_bk ? 2 * p.B : p.B;
        if (p.min_s)
            expect_kernel<K, D, NW, true><<<blocks, 64 * NW, 0, stream>>>(p, with_bk, expected);
        else
            expect_kernel<K, D, NW, false><<<blocks, 64 * NW, 0, stream>>>(p, with_bk, expected);
    }
};

// ---- gradient ------------------------------------------------------------------------------------------------------

// The expected cost's rows for the shared streamers (mrnnt_grad.h): band = the loss's band; a row's two weights from
// alpha / beta / A / Bk / lp / ll / R, the two costs and the two upstream scalars; the other rows exact zeros -- NaN
// for an utterance whose ll is not finite. Slot, formula and scalar twin: WeightRows.
struct ExpectRows : WeightRows {
    struct Col {
        int T, lo, hi;
        bool fin;
        double ll, R;
        float ge, gc;
        int64_t arow;  // the column's first row in the cost arrays (acts' row layout)
    };
    static __device__ __forceinline__ Col column(const DevProblem &p, int b, int64_t, int t, int T, int S) {
        Col c;
        c.T = T;
        c.lo = max(0, t - (T - S));
        c.hi = min(t, S);
        c.ll = p.ll[b];
        c.fin = __builtin_isfinite(c.ll);
        c.R = p.ex_R[b];
        c.ge = p.ex_ge ? p.ex_ge[b] : 0.0f;
        c.gc = p.ex_gc ? p.ex_gc[b] : 0.0f;
        c.arow = acts_col_base(p, b, t, p.row_off[b] + (int64_t)t * (S + 1));
        return c;
    }
    static __device__ __forceinline__ float zero(const Col &col, float) { return col.fin ? 0.0f : __builtin_nanf(""); }

    // (as row_coef: nothing of the row is read before it is known to be in the band and reachable -- under a
    // restricting alignment lp is written only inside the alignment window)
    static __device__ __forceinline__ Slot stage(const DevProblem &p, const Col &col, int t, int S, int s, int64_t rowc,
                                                 const int *lab_b) {
        Slot c{0.0f, 0.0f, 0.0f, 0.0f, kDeadRow};
        if (!col.fin || !(s >= col.lo && s <= col.hi)) return c;
        const int W = S + 1;
        const int64_t row = rowc + s;
        const double base = alpha_prev(p, t, s, row, W) - col.ll;
        if (!row_live(base + p.beta[row])) return c;
        const bool last = t == col.T - 1;
        const double b1 = last ? (s == S ? 0.0 : NEG_INF_D) : p.beta[row + W];
        const double b2 = (s == S) ? NEG_INF_D : (last ? (s + 1 == S ? 0.0 : NEG_INF_D) : p.beta[row + W + 1]);
        const Lp l = p.lp[row];
        // the two arc posteriors as row_coef forms them (fp64 cancellation, then v_exp_f32: relative error ~1e-6)
        const float pb = fast_exp2((float)((l.b + base + b1) * kLog2eD));
        const float pe = (s < S) ? fast_exp2((float)((l.e + base + b2) * kLog2eD)) : 0.0f;
        const double ap = (t == 0) ? 0.0 : p.ex_A[row - W];
        double wb = 0.0, we = 0.0;
        if (pb != 0.0f) {  // (deviation of the paths through the arc from the mean: the fp64 cancellation first)
            const double dev = ap + (p.ex_wb ? (double)p.ex_wb[col.arow + s] : 0.0) + (last ? 0.0 : p.ex_Bk[row + W]) - col.R;
            wb = (double)pb * ((double)col.gc - (double)col.ge * dev);
        }
        if (pe != 0.0f) {
            const double dev =
                ap + (p.ex_we ? (double)p.ex_we[col.arow + s] : 0.0) + (last ? 0.0 : p.ex_Bk[row + W + 1]) - col.R;
            we = (double)pe * ((double)col.gc - (double)col.ge * dev);
        }
        c.cb = (float)wb;
        c.ce = (float)we;
        if (c.cb == 0.0f && c.ce == 0.0f) return c;  // (lab is still kDeadRow: exact zeros, acts not read)
        c.c2 = p.den[row] * kLog2e;
        c.wocc = (float)(wb + we);
        c.lab = slot_label(p, S, s, lab_b);
        return c;
    }
    static __device__ __forceinline__ bool row(const DevProblem &p, const Col &col, int t, int S, int s, int64_t rowc,
                                               const int *lab_b, Coef &c) {
        c = stage(p, col, t, S, s, rowc, lab_b);
        return live(c);
    }

    // every live in-band row is read, as by the loss: the acts loads go nontemporal by size
    static constexpr bool kNtLoads = true;
    template <class IO, bool NTL, bool NTS, int U>
    static void launch_u(const DevProblem &p, const float *, void *grads, int grid, hipStream_t stream) {
        grad_staged_kernel<IO, U, staged_rows(U), NTL, NTS, ExpectRows><<<grid, 256, 0, stream>>>(p, nullptr, grads);
    }
};

}  // namespace

hipError_t launch_expect(const DevProblem &p, int S_max, int with_bk, float *expected, hipStream_t stream) {
    if (!launch_by_width<true>(S_max + 1, ExpectLaunch{p, with_bk, expected, stream})) return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_expect_grad(const DevProblem &p, int elem, void *grads, int grid, hipStream_t stream) {
    return launch_grad_rows<ExpectRows>(p, elem, nullptr, grads, grid, stream);
}

}  // namespace mrnnt
