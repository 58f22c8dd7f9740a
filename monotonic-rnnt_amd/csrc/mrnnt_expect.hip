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
// The fused joint (mrnnt_joint_expect_*) has no dense gradient: expect_coef_kernel writes the same Wb / We -- one
// function, expect_weights, forms them for both -- of every in-band row into two arrays, from which mrnnt_joint.hip
// lists the rows that have any and runs its MFMA gradient pass with the path scores' coefficients.
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

// The two weights of an in-band row (t, s) of g_e . expected + g_c . costs, in fp64 -- shared by the dense gradient
// (ExpectRows::stage) and the fused joint's coefficient launch (expect_coef_kernel):
//   Wb = blank_post (g_c - g_e (A(t-1, s) + wb + Bk(t+1, s)   - R))
//   We = label_post (g_c - g_e (A(t-1, s) + we + Bk(t+1, s+1) - R))      (0 at s = S: label_arc false)
// the posteriors as row_coef forms them, the deviation from the mean in fp64 first; {0, 0} for a row no path reaches
// (kDeadLogOcc), decided before anything else of the row is asked for. Src hands over the row's inputs one by one:
// RowInMemory loads each where it is first needed (nothing of a dead row but alpha / beta is read -- under a
// restricting alignment lp is written only inside the alignment window), RowLoaded holds values loaded ahead.
struct ArcWeights {
    double wb, we;
};

template <class Src>
__device__ __forceinline__ ArcWeights expect_weights(const Src &r, bool label_arc, double ll, double R, float ge,
                                                     float gc) {
    ArcWeights w{0.0, 0.0};
    const double base = r.a_prev() - ll;
    if (!row_live(base + r.beta0())) return w;
    const double b1 = r.beta_blank();
    const double b2 = r.beta_label();
    const Lp l = r.lp();
    // the two arc posteriors as row_coef forms them (fp64 cancellation, then v_exp_f32: relative error ~1e-6)
    const float pb = fast_exp2((float)((l.b + base + b1) * kLog2eD));
    const float pe = label_arc ? fast_exp2((float)((l.e + base + b2) * kLog2eD)) : 0.0f;
    const double ap = r.A_prev();
    if (pb != 0.0f) {  // (deviation of the paths through the arc from the mean: the fp64 cancellation first)
        const double dev = ap + r.cost_blank() + r.Bk_blank() - R;
        w.wb = (double)pb * ((double)gc - (double)ge * dev);
    }
    if (pe != 0.0f) {
        const double dev = ap + r.cost_label() + r.Bk_label() - R;
        w.we = (double)pe * ((double)gc - (double)ge * dev);
    }
    return w;
}

struct RowInMemory {
    const DevProblem &p;
    int t, S, s, W;
    int64_t row, arow;  // the lattice row; the column's first row in the cost arrays (acts' row layout)
    bool last;          // t == T - 1
    __device__ __forceinline__ double a_prev() const { return alpha_prev(p, t, s, row, W); }
    __device__ __forceinline__ double beta0() const { return p.beta[row]; }
    __device__ __forceinline__ double beta_blank() const {
        return last ? (s == S ? 0.0 : NEG_INF_D) : p.beta[row + W];
    }
    __device__ __forceinline__ double beta_label() const {
        return (s == S) ? NEG_INF_D : (last ? (s + 1 == S ? 0.0 : NEG_INF_D) : p.beta[row + W + 1]);
    }
    __device__ __forceinline__ Lp lp() const { return p.lp[row]; }
    __device__ __forceinline__ double A_prev() const { return (t == 0) ? 0.0 : p.ex_A[row - W]; }
    __device__ __forceinline__ double cost_blank() const { return p.ex_wb ? (double)p.ex_wb[arow + s] : 0.0; }
    __device__ __forceinline__ double cost_label() const { return p.ex_we ? (double)p.ex_we[arow + s] : 0.0; }
    __device__ __forceinline__ double Bk_blank() const { return last ? 0.0 : p.ex_Bk[row + W]; }
    __device__ __forceinline__ double Bk_label() const { return last ? 0.0 : p.ex_Bk[row + W + 1]; }
};

struct RowLoaded {
    double am, b0, b1, b2, ap, k1, k2;
    Lp l;
    float cwb, cwe;
    __device__ __forceinline__ double a_prev() const { return am; }
    __device__ __forceinline__ double beta0() const { return b0; }
    __device__ __forceinline__ double beta_blank() const { return b1; }
    __device__ __forceinline__ double beta_label() const { return b2; }
    __device__ __forceinline__ Lp lp() const { return l; }
    __device__ __forceinline__ double A_prev() const { return ap; }
    __device__ __forceinline__ double cost_blank() const { return (double)cwb; }
    __device__ __forceinline__ double cost_label() const { return (double)cwe; }
    __device__ __forceinline__ double Bk_blank() const { return k1; }
    __device__ __forceinline__ double Bk_label() const { return k2; }
};

// The fused joint's coefficient launch (mrnnt_joint_expect_rows): Wb / We of every row of the monotonic band into
// out_b / out_e (fp64 [N], the lattice's packed rows), for the expect-live row list (launch_row_list mode 3) and the
// MFMA gradient pass (PathCoef reads them as p.alpha / p.beta). One wave per lattice column, lanes along s, grid-stride
// over columns. A row whose two weights round to fp32 zeros -- what the gradient pass would stage -- holds exact 0.0
// (dead, unreachable, outside a restricting alignment's window, underflow): it is not listed. Every in-band row of an
// utterance whose ll is not finite holds NaN. Rows outside the band are not written.
// The loads of a row do not depend on one another and none sits behind a branch: a lane past the band's end, the
// first / last frame and s = S load a clamped address (the row itself, or the band's last row) and the boundary value
// is selected afterwards, so the ten loads are issued together and waited for once (build_row's rule, mrnnt_joint_tile.h).
// Everything they touch is allocated and initialised: alpha / beta / A / Bk over the band, lp zero-filled by the joint
// forward, the cost arrays over the caller's grid (the label cost of s = S_b is addressed at s = S_b - 1; a value the
// contract calls never-read -- S_b = 0, a dead row -- may be loaded and is then dropped by a select, never multiplied).
template <bool WB, bool WE>
__global__ __launch_bounds__(256) void expect_coef_kernel(DevProblem p, double *__restrict__ out_b,
                                                          double *__restrict__ out_e) {
    if (p.dyn && __builtin_amdgcn_readfirstlane(p.dyn->status)) return;  // failed lengths: nothing is touched
    const int lane = threadIdx.x & 63;
    for (int64_t col = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); col < p.num_cols; col += (int64_t)gridDim.x * 4) {
        const int b = p.col_b[col];
        const int T = p.T[b], S = p.S[b], W = S + 1;
        const int t = (int)(col - p.col_off[b]);
        const int64_t rowc = p.row_off[b] + (int64_t)t * W;
        const int lo = max(0, t - (T - S)), hi = min(t, S);
        const double ll = p.ll[b], R = p.ex_R[b];
        const float ge = p.ex_ge ? p.ex_ge[b] : 0.0f, gc = p.ex_gc ? p.ex_gc[b] : 0.0f;
        const bool fin = __builtin_isfinite(ll), first = t == 0, last = t == T - 1;
        const int64_t arow = acts_col_base(p, b, t, rowc);
        const int64_t up = first ? 0 : -(int64_t)W, dn = last ? 0 : (int64_t)W;  // the neighbour frames, clamped
        for (int s0 = lo; s0 <= hi; s0 += 64) {
            const bool in = s0 + lane <= hi;
            const int s = min(s0 + lane, hi);  // lanes past the band work on its last row and store nothing
            const int sn = min(s + 1, S);
            const int64_t row = rowc + s;
            RowLoaded r;
            r.am = p.alpha[row + up];
            r.b0 = p.beta[row];
            r.b1 = p.beta[row + dn];
            r.b2 = p.beta[rowc + dn + sn];
            r.l = p.lp[row];
            r.ap = p.ex_A[row + up];
            r.k1 = p.ex_Bk[row + dn];
            r.k2 = p.ex_Bk[rowc + dn + sn];
            r.cwb = WB ? p.ex_wb[arow + s] : 0.0f;
            r.cwe = WE ? p.ex_we[arow + max(min(s, S - 1), 0)] : 0.0f;
            if (first) {
                r.am = s == 0 ? 0.0 : NEG_INF_D;
                r.ap = 0.0;
            }
            if (last) {
                r.b1 = s == S ? 0.0 : NEG_INF_D;
                r.b2 = s + 1 == S ? 0.0 : NEG_INF_D;
                r.k1 = r.k2 = 0.0;
            }
            if (s == S) r.b2 = NEG_INF_D;
            ArcWeights w = expect_weights(r, s < S, ll, R, ge, gc);
            if ((float)w.wb == 0.0f && (float)w.we == 0.0f) w.wb = w.we = 0.0;
            if (!fin) w.wb = w.we = __builtin_nan("");
            if (in) {
                out_b[row] = w.wb;
                out_e[row] = w.we;
            }
        }
    }
}

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
        const int64_t row = rowc + s;
        const RowInMemory r{p, t, S, s, S + 1, row, col.arow, t == col.T - 1};
        const ArcWeights w = expect_weights(r, s < S, col.ll, col.R, col.ge, col.gc);
        c.cb = (float)w.wb;
        c.ce = (float)w.we;
        if (c.cb == 0.0f && c.ce == 0.0f) return c;  // (lab is still kDeadRow: exact zeros, acts not read)
        c.c2 = p.den[row] * kLog2e;
        c.wocc = (float)(w.wb + w.we);
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

// The factorised-blank twin (mrnnt_hat_expect_backward, after mrnnt_hat_expect_forward): ExpectRows' band, zero value
// and weights -- expect_weights reads alpha / beta / lp / A / Bk, never a logit, so it serves unchanged -- with
// HatWeightRows' slot and formula. Dead where both fp32 weights are zero, as ExpectRows.
struct HatExpectRows : HatWeightRows {
    typedef ExpectRows::Col Col;
    static __device__ __forceinline__ Col column(const DevProblem &p, int b, int64_t c, int t, int T, int S) {
        return ExpectRows::column(p, b, c, t, T, S);
    }
    static __device__ __forceinline__ float zero(const Col &col, float sc) { return ExpectRows::zero(col, sc); }

    static __device__ __forceinline__ Slot stage(const DevProblem &p, const Col &col, int t, int S, int s, int64_t rowc,
                                                 const int *lab_b) {
        if (!col.fin || !(s >= col.lo && s <= col.hi)) return dead();
        const int64_t row = rowc + s;
        const RowInMemory r{p, t, S, s, S + 1, row, col.arow, t == col.T - 1};
        const ArcWeights w = expect_weights(r, s < S, col.ll, col.R, col.ge, col.gc);
        if ((float)w.wb == 0.0f && (float)w.we == 0.0f) return dead();  // exact zeros, acts not read
        return weight_slot(p, S, s, row, w.wb, w.we, lab_b);
    }
    static __device__ __forceinline__ bool row(const DevProblem &p, const Col &col, int t, int S, int s, int64_t rowc,
                                               const int *lab_b, Coef &c) {
        const Slot cf = stage(p, col, t, S, s, rowc, lab_b);
        c = coef(cf);
        return live(cf);
    }

    static constexpr bool kNtLoads = true;
    template <class IO, bool NTL, bool NTS, int U>
    static void launch_u(const DevProblem &p, const float *, void *grads, int grid, hipStream_t stream) {
        grad_staged_kernel<IO, U, staged_rows(U), NTL, NTS, HatExpectRows><<<grid, 256, 0, stream>>>(p, nullptr, grads);
    }
};

}  // namespace

hipError_t launch_hat_expect_grad(const DevProblem &p, int elem, void *grads, int grid, hipStream_t stream) {
    return launch_grad_rows<HatExpectRows>(p, elem, nullptr, grads, grid, stream);
}

hipError_t launch_expect(const DevProblem &p, int S_max, int with_bk, float *expected, hipStream_t stream) {
    if (!launch_by_width<true>(S_max + 1, ExpectLaunch{p, with_bk, expected, stream})) return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_expect_coef(const DevProblem &p, double *wb_out, double *we_out, hipStream_t stream) {
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((p.num_cols + 3) / 4, 1 << 20));
    if (p.ex_wb && p.ex_we)
        expect_coef_kernel<true, true><<<blocks, 256, 0, stream>>>(p, wb_out, we_out);
    else if (p.ex_wb)
        expect_coef_kernel<true, false><<<blocks, 256, 0, stream>>>(p, wb_out, we_out);
    else if (p.ex_we)
        expect_coef_kernel<false, true><<<blocks, 256, 0, stream>>>(p, wb_out, we_out);
    else
        expect_coef_kernel<false, false><<<blocks, 256, 0, stream>>>(p, wb_out, we_out);
    return hipGetLastError();
}

hipError_t launch_expect_grad(const DevProblem &p, int elem, void *grads, int grid, hipStream_t stream) {
    return launch_grad_rows<ExpectRows>(p, elem, nullptr, grads, grid, stream);
}

}  // namespace mrnnt
