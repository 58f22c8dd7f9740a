// mrnnt_joint.hip -- the joint network fused into the loss ("fusing the joint network's
// final projection with the softmax pass so the N x V tensor is never materialised").
//
//   z(b,t,s,:) = W * tanh(enc[b,t,:] + pred[b,s,:]) + bias          (W: [V, H] bf16, fp32 accumulate)
//
// The packed logits the reference's loss takes as `acts` (monotonic_rnnt_op.py:133-140) are formed on MFMA
// (v_mfma_f32_32x32x16_bf16) tile by tile inside two passes and never written to HBM:
//   forward  : per in-band lattice row the log-softmax denominator and the blank / label log-probs (what
//              mrnnt_softmax.hip computes from stored acts), then the unchanged alpha/beta recursion;
//   backward : per LIVE row (the occupancy-skip predicate of mrnnt_grad.hip) the logit gradient
//              g = dL/dz (bf16) and the joint activation tanh(enc + pred) (bf16), so that dW = G^T Hact,
//              dH = G W and dbias = sum G are plain GEMMs / reductions over live rows only.
//
// Tiling: a workgroup of 8 waves (two per SIMD) owns 256 consecutive rows of a row list; a wave owns 32 rows and
// keeps their activations as the MFMA B operand in registers (lane l: row l&31, k = 16 ks + 8 (l>>5) + [0,8)),
// built once from enc/pred with a fast tanh. W streams through LDS in 32-vocabulary chunks (LDS-DMA, double-
// buffered, XOR-swizzled against bank conflicts) shared by the 8 waves; each chunk is one 32x32 output tile per wave,
// D[vocab][row] = sum_k W[vocab][k] h[row][k]: the accumulator holds 16 vocabulary entries of ONE row per
// lane (vocab = (i&3) + 8 (i>>2) + 4 (l>>5)), so the per-row online softmax is register-local and the two
// lane halves merge once at the end.
#include <algorithm>

#include "mrnnt_hat.h"  // HatCoef / hat_coef (the factorised-blank row coefficients)
#include "mrnnt_joint_tile.h"
#include "mrnnt_lsm.h"  // hat_lp (the factorised-blank log-probs of a row)

namespace mrnnt {

// two waves per SIMD: the compiler keeps each kernel within 256 registers per lane
// TR: the development build's timeline stamps (JOINT_MARK), instantiated only when the joint_trace knob asks for them:
// the stamps (a scalar clock read and a store per mark, one inside the chunk loop) cost that build's forward ~15 %
// HAT: the factorised-blank flavour (mrnnt_joint_hat_*, chosen on the host from DevProblem::hat): den' = -LSE over the
// non-blank logits and hat_lp's pair (mrnnt_lsm.h, the helper of the acts kernels). The blank logit never enters the
// max or the sum: its chunk is wave-uniform, the lane and register that hold it are acc_reg_of's, and in that chunk
// that register's term is -inf before the max and before the exp (drop_reg) -- in all three epilogue forms. Subtracting
// exp(z_b) from a sum over the whole row instead cancels to nothing once z_b dominates (z_b = +55 in the plain form,
// inside the +-64 bound). The plain sum stays safe with one term fewer, so joint_wbound_kernel decides as before.
template <int KS, int NB, int NW, int RG, bool TR = false, bool HAT = false>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(2, 2))) void joint_fwd_kernel(DevProblem p,
                                                                                             JointArgs j) {
    extern __shared__ __attribute__((aligned(16))) unsigned short wsh[];
    if ((int64_t)blockIdx.x * (32 * NW) >= list_len(j)) return;  // whole workgroup past a shorter list
    FWD_MARK(0);
    const int lane = threadIdx.x & 63, half = lane >> 5;
    const int64_t i = (int64_t)blockIdx.x * (32 * NW) + (threadIdx.x >> 6) * 32 + (lane & 31);
    const RowPos q = row_pos(p, j, i);
    const int V = p.V, blank = p.blank;
    const float *bias = load_bias<KS, NB>(j, V, wsh, (j.opt & 2) != 0);
    __syncthreads();
    FWD_MARK(1);
    bf16x8 bfr[KS];
    build_act<KS, false>(j, q, half, i, bfr);
    FWD_MARK(2);

    const f2 l2e = {kLog2e, kLog2e};
    float m = NEG_INF_F, sum = 0.0f, zb = 0.0f, ze = 0.0f;
    bool fb = false, fe = false;
    // the blank / label logits of this lane's half of chunk c (the same selects in both epilogues)
    auto capture = [&](const f2 (&z)[8], int c) {
        const int jb = blank - 32 * c;  // wave-uniform: one chunk holds the blank
        if (jb >= 0 && jb < 32) {
            const int rb = acc_reg_of(jb, half);
            if (rb >= 0) {
                zb = tree_pick(z, rb);
                fb = true;
            }
        }
        const int jl = q.lab - 32 * c;
        const int rl = acc_reg_of(jl & 31, half);
        const bool mine = q.lab >= 0 && jl >= 0 && jl < 32 && rl >= 0;
        if (__ballot(mine)) {  // most chunks hold some lane's label; skip the select when none does
            const float x = tree_pick(z, rl);
            if (mine) {
                ze = x;
                fe = true;
            }
        }
    };
    // HAT: the blank's term out of x, in the blank's chunk only (wave-uniform: sixteen selects in one chunk of the row).
    // The guard is spelled on blank itself, not as in_chunk() (on blank - 32 c), on purpose: the compiler does not
    // take the two for the same test, and in_chunk here reschedules the HAT forward from its first lines on.
    auto drop_blank = [&](f2 (&x)[8], int c) {
        if (blank >= 32 * c && blank < 32 * c + 32) drop_reg(x, blank_reg(blank, c, half));
    };
    // the two lane halves hold the same row and disjoint vocabulary: whichever captured the blank / label logit has it
    auto merge_captured = [&]() {
        const float zb2 = __shfl_xor(zb, 32), ze2 = __shfl_xor(ze, 32);
        const int fb2 = __shfl_xor((int)fb, 32), fe2 = __shfl_xor((int)fe, 32);
        if (!fb && fb2) zb = zb2;
        if (!fe && fe2) ze = ze2;
    };
    // the row's outputs from its denominator; an out-of-range label is NaN, and for HAT (den' over the non-blank logits)
    // a label equal to blank is no arc
    auto write_row = [&](double den) {
        p.den[q.row] = (float)den;
        if constexpr (HAT) {
            const float zl = q.lab == blank ? NEG_INF_F : (q.lab >= 0 ? ze : (q.lab == -2 ? __builtin_nanf("") : 0.0f));
            p.lp[q.row] = hat_lp(zb, zl, den);
        } else {
            p.lp[q.row] = Lp{(double)zb + den, (q.lab >= 0 ? (double)ze : (q.lab == -2 ? __builtin_nan("") : 0.0)) + den};
        }
    };
    // Bounded weights (j.wplain: |z| <= 64 for every logit, joint_wbound_kernel): a plain exp-sum -- 1024 terms of
    // at most e^64 cannot overflow fp32 and the largest cannot underflow -- without the running max, whose
    // per-chunk max / rescale chain cost 15 % of the forward. Otherwise the online log-sum-exp.
    const bool plain = j.wplain != nullptr && *j.wplain != 0;
    if (plain && (j.opt & 2)) {
        // exp2(fma(acc, log2 e, bias log2 e)) from a prescaled bias row (bias2, after the bias row in LDS): one fma per
        // logit where the bias add and the log2 e multiply were two; the captured blank / label logits are still
        // acc + bias (picked from the accumulator, the bias added to the picked value: the same fp32 add)
        const float *bias2 = bias + vpad(V);
        chunk_loop<KS, NB, NW, RG, TR>(j, V, wsh, bfr, lane, 0, [&](const f32x16 &acc, int c) {
            // (two bodies on purpose: summing as each pair of terms is formed, and forming all sixteen first as the
            // drop needs, schedule the non-HAT chunk loop differently; a single body has to be cleared by timing)
            f2 s2 = {0.0f, 0.0f};
            f2 a2[8];
            if constexpr (HAT) {
                f2 t[8];
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const f4 bv = *reinterpret_cast<const f4 *>(bias2 + 32 * c + 8 * q4 + 4 * half);
                    a2[2 * q4] = (f2){acc[4 * q4], acc[4 * q4 + 1]};
                    a2[2 * q4 + 1] = (f2){acc[4 * q4 + 2], acc[4 * q4 + 3]};
                    t[2 * q4] = fma2(a2[2 * q4], l2e, (f2){bv.x, bv.y});
                    t[2 * q4 + 1] = fma2(a2[2 * q4 + 1], l2e, (f2){bv.z, bv.w});
                }
                drop_blank(t, c);
#pragma unroll
                for (int k = 0; k < 8; ++k) s2 = add2(s2, (f2){fast_exp2(t[k].x), fast_exp2(t[k].y)});
            } else {
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const f4 bv = *reinterpret_cast<const f4 *>(bias2 + 32 * c + 8 * q4 + 4 * half);
                    a2[2 * q4] = (f2){acc[4 * q4], acc[4 * q4 + 1]};
                    a2[2 * q4 + 1] = (f2){acc[4 * q4 + 2], acc[4 * q4 + 3]};
                    const f2 t0 = fma2(a2[2 * q4], l2e, (f2){bv.x, bv.y});
                    const f2 t1 = fma2(a2[2 * q4 + 1], l2e, (f2){bv.z, bv.w});
                    s2 = add2(s2, (f2){fast_exp2(t0.x), fast_exp2(t0.y)});
                    s2 = add2(s2, (f2){fast_exp2(t1.x), fast_exp2(t1.y)});
                }
            }
            sum += s2.x + s2.y;
            const int jb = blank - 32 * c;
            if (jb >= 0 && jb < 32) {
                const int rb = acc_reg_of(jb, half);
                if (rb >= 0) {
                    zb = tree_pick(a2, rb) + bias[32 * c + jb];
                    fb = true;
                }
            }
            const int jl = q.lab - 32 * c;
            const int rl = acc_reg_of(jl & 31, half);
            const bool mine = q.lab >= 0 && jl >= 0 && jl < 32 && rl >= 0;
            if (__ballot(mine)) {
                const float x = tree_pick(a2, rl) + bias[32 * c + (jl & 31)];
                if (mine) {
                    ze = x;
                    fe = true;
                }
            }
            if (c == 0) FWD_MARK(3);
        });
    } else if (plain) {
        chunk_loop<KS, NB, NW, RG, TR>(j, V, wsh, bfr, lane, 0, [&](const f32x16 &acc, int c) {
            f2 z[8];
            logits2(acc, bias, c, half, z);
            if constexpr (HAT) {  // z_b picked first, then out of the row
                capture(z, c);
                drop_blank(z, c);
            }
            f2 s2 = {0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const f2 t = mul2(z[k], l2e);
                s2 = add2(s2, (f2){fast_exp2(t.x), fast_exp2(t.y)});
            }
            sum += s2.x + s2.y;
            if constexpr (!HAT) capture(z, c);
            if (c == 0) FWD_MARK(3);
        });
    }
    if (plain) {
        sum += __shfl_xor(sum, 32);
        merge_captured();
        if (q.valid && half == 0) write_row(-log_row_sum(sum));
        FWD_MARK(4);
        return;
    }
    chunk_loop<KS, NB, NW, RG, TR>(j, V, wsh, bfr, lane, 0, [&](const f32x16 &acc, int c) {
        f2 z[8];
        logits2(acc, bias, c, half, z);
        if constexpr (HAT) {  // z_b picked first, then out of the row before this chunk's max
            capture(z, c);
            drop_blank(z, c);
        }
        float cm = fmaxf(z[0].x, z[0].y);
#pragma unroll
        for (int k = 1; k < 8; ++k) cm = max3(cm, z[k].x, z[k].y);
        const float mn = fmaxf(m, cm);
        const float mr = (mn == NEG_INF_F) ? 0.0f : mn;
        const f2 nb = {-mr * kLog2e, -mr * kLog2e};
        f2 s2 = {0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const f2 t = fma2(z[k], l2e, nb);
            s2 = add2(s2, (f2){fast_exp2(t.x), fast_exp2(t.y)});
        }
        sum = sum * fast_exp2((m - mr) * kLog2e) + (s2.x + s2.y);
        m = mn;
        if constexpr (!HAT) capture(z, c);
        if (c == 0) FWD_MARK(3);
    });
    // merge the two lane halves (same row, disjoint vocabulary)
    const float m2 = __shfl_xor(m, 32), s2 = __shfl_xor(sum, 32);
    const float mn = fmaxf(m, m2);
    const float mr = (mn == NEG_INF_F) ? 0.0f : mn;
    sum = sum * fast_exp2((m - mr) * kLog2e) + s2 * fast_exp2((m2 - mr) * kLog2e);
    merge_captured();
    if (q.valid && half == 0) write_row(-(double)mn - log_row_sum(sum));
    FWD_MARK(4);
}

#ifdef MRNNT_DEVTOOLS
__device__ unsigned long long g_joint_trace[kJointTraceWgs * 64];  // (JOINT_MARK's timeline, mrnnt_joint_tile.h)

int joint_trace(unsigned long long *out, int n) {
    n = std::min(n, kJointTraceWgs * 64);
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_joint_trace), sizeof(unsigned long long) * n) != hipSuccess) return -1;
    return n;
}
#endif

// Row coefficients of the MFMA gradient kernels (the policy mrnnt_grad.h gives the streaming kernels): what a list row
// stages once, and what the chunk epilogue makes of e = exp2(z log2 e + c2) -- a plain entry, the row's blank / label
// entry, and the two corrections' share of the dbias column sums.
// The loss: g = scale * (softmax occupancy - corrections), coefficients from alpha / beta / ll (row_coef).
struct LossCoef {
    float c2, cb, ce, sc;
    int lab;
    __device__ __forceinline__ void clear() {
        c2 = cb = ce = sc = 0.0f;
        lab = -1;
    }
    __device__ __forceinline__ void stage(const DevProblem &p, const JointArgs &j, const RowPos &q) {
        const RowCoef rc =
            row_coef(p, q.t, q.T, q.S, q.s, q.row, p.ll[q.b], p.labels + (int64_t)q.b * p.label_stride);
        c2 = rc.c2, cb = rc.cb, ce = rc.ce, lab = rc.lab;
        sc = j.scale ? j.scale[q.b] : 1.0f;
    }
    __device__ __forceinline__ float out(float e) const { return e * sc; }
    __device__ __forceinline__ float out_blank(float e) const { return (e - cb) * sc; }
    __device__ __forceinline__ float out_label(float e) const { return (e - ce) * sc; }
    // what the dbias column sum, which holds out(e) for every entry, loses at the row's blank / label entry (e: the
    // blank entry's value, for a policy whose blank element does not follow from it)
    __device__ __forceinline__ float sum_blank(float) const { return cb * sc; }
    __device__ __forceinline__ float sum_label() const { return ce * sc; }
    static constexpr bool kHat = false;
};

// Path scores (mrnnt_joint_path_backward): g = wocc * softmax - [blank] Wb - [label] We, the formula of PathRows::grad
// (mrnnt_path.hip), with Wb / We in p.alpha / p.beta (launch_path_coef) and den from the forward. wocc = Wb + We is a
// signed multiplier -- never a divisor: wocc = 0 with Wb = -We != 0 is a live row whose two corrections stay. Only
// listed rows are staged (path-live: inside the hull), so nothing uninitialised is read.
// Expected costs (mrnnt_joint_expect_backward) run the same class over the expect-live rows: their launch's p.alpha /
// p.beta point at launch_expect_coef's two arrays.
struct PathCoef {
    float c2, wocc, cb, ce;
    int lab;
    __device__ __forceinline__ void clear() {
        c2 = wocc = cb = ce = 0.0f;
        lab = -1;
    }
    __device__ __forceinline__ void stage(const DevProblem &p, const JointArgs &, const RowPos &q) {
        const double wb = p.alpha[q.row], we = p.beta[q.row];
        c2 = p.den[q.row] * kLog2e;
        wocc = (float)(wb + we);
        cb = (float)wb;
        ce = (float)we;
        lab = (q.lab < 0 || q.lab == p.blank) ? -1 : q.lab;  // (s == S, out of range, label == blank: as row_coef)
    }
    __device__ __forceinline__ float out(float e) const { return wocc * e; }
    __device__ __forceinline__ float out_blank(float e) const { return wocc * e - cb; }
    __device__ __forceinline__ float out_label(float e) const { return wocc * e - ce; }
    __device__ __forceinline__ float sum_blank(float) const { return cb; }
    __device__ __forceinline__ float sum_label() const { return ce; }
    static constexpr bool kHat = false;
};

// The factorised blank (mrnnt_joint_hat_backward): the coefficients of hat_coef (mrnnt_hat.h, the definition HatRows
// streams stored logits with), g[v != b] = sc (exp2(z log2 e + c2) - [v == label] ce) with ce folded into c2, and the
// blank element sc gb -- gb = ce sigmoid(z_b) - cb sigmoid(-z_b), formed once per row from lpb -- whatever e is.
// kHat: the kernels take the blank logit out of the row before the exp (-inf in its register, in its chunk only), so
// the blank entry's e is exactly 0 -- not exp(z_b + den' + log ce), which overflows fp32 once the blank dominates the
// row -- and the dbias column sum, which holds out(0) = 0 there, is corrected to sc gb by sum_blank.
struct HatJointCoef {
    float c2, ce, gb, sc;
    int lab;
    __device__ __forceinline__ void clear() {
        c2 = ce = gb = sc = 0.0f;
        lab = -1;
    }
    __device__ __forceinline__ void stage(const DevProblem &p, const JointArgs &j, const RowPos &q) {
        HatCoef rc;
        const double ll = p.ll[q.b];
        hat_coef(p, q.t, q.T, q.S, q.s, q.row, ll, p.labels + (int64_t)q.b * p.label_stride, rc);
        c2 = rc.c2, ce = rc.ce, gb = rc.gb, lab = rc.lab;
        // An utterance without a path (ll = -inf, cost +inf: e.g. every label masked by a -inf bias) has no arc
        // posteriors, and exp(... - ll) is NaN in every coefficient. Its rows come out exact zeros here: d_weight and
        // d_bias sum over the batch, and one such utterance must not turn the other utterances' share of them into
        // NaN. (A NaN ll -- a NaN / +inf logit -- keeps its NaN gradients.)
        if (ll == NEG_INF_D) {
            c2 = NEG_INF_F;
            ce = gb = 0.0f;
        }
        sc = j.scale ? j.scale[q.b] : 1.0f;
    }
    __device__ __forceinline__ float out(float e) const { return e * sc; }
    __device__ __forceinline__ float out_blank(float) const { return gb * sc; }
    __device__ __forceinline__ float out_label(float e) const { return (e - ce) * sc; }
    __device__ __forceinline__ float sum_blank(float e) const { return out(e) - gb * sc; }
    __device__ __forceinline__ float sum_label() const { return ce * sc; }
    static constexpr bool kHat = true;
};

template <int KS, int NB, int NW, int RG, class RC>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(2, 2))) void joint_bwd_kernel(DevProblem p,
                                                                                             JointArgs j) {
    extern __shared__ __attribute__((aligned(16))) unsigned short wsh[];
    if (j.n_dev && (int64_t)blockIdx.x * (32 * NW) >= list_len(j)) return;  // past the device count (tail zeroed)
    const int lane = threadIdx.x & 63, half = lane >> 5;
    const int64_t i = (int64_t)blockIdx.x * (32 * NW) + (threadIdx.x >> 6) * 32 + (lane & 31);
    const RowPos q = row_pos(p, j, i);
    RC rc;
    rc.clear();
    if (q.valid) {
        rc.stage(p, j, q);
        if (half == 0 && j.bt_idx) j.bt_idx[i] = (int64_t)q.b * (j.enc_sb / j.H) + q.t;
        if (half == 0 && j.bs_idx) j.bs_idx[i] = (int64_t)q.b * (j.pred_sb / j.H) + q.s;
    }
    const int V = p.V, blank = p.blank;
    const float *bias = load_bias<KS, NB>(j, V, wsh);
    __syncthreads();
    bf16x8 bfr[KS];
    build_act<KS, true>(j, q, half, i, bfr);

    // exactly 4 vector stores per chunk on every wave with a valid lane: leave them in flight at the barrier
    const bool vec_out = (V & 3) == 0;
    const bool leave = vec_out && __ballot(!q.valid) == 0;
    unsigned short *grow = j.G + (q.valid ? i : 0) * V;
    const f2 l2e = {kLog2e, kLog2e}, c2 = {rc.c2, rc.c2};
    chunk_loop<KS, NB, NW, RG>(j, V, wsh, bfr, lane, leave ? 4 : -1, [&](const f32x16 &acc, int c) {
        f2 g[8];
        logits2(acc, bias, c, half, g);
        const int rb = blank_reg(blank, c, half);
        if constexpr (RC::kHat)  // the blank logit out of the row before the exp: its entry's e is 0
            if (in_chunk(blank, c)) drop_reg(g, rb);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const f2 t = fma2(g[k], l2e, c2);
            g[k] = (f2){fast_exp2(t.x), fast_exp2(t.y)};
        }
        // the <= 2 corrected entries of the row are rewritten by a second (2-byte) store after the vector store
        const int jl = rc.lab - 32 * c;
        const int rl = acc_reg_of(jl & 31, half);
        const bool mine = rc.lab >= 0 && jl >= 0 && jl < 32 && rl >= 0;
        float gb = 0.0f, gl = 0.0f;
        if (rb >= 0) gb = tree_pick(g, rb);
        if (__ballot(mine)) gl = tree_pick(g, rl);
#pragma unroll
        for (int k = 0; k < 8; ++k) g[k] = (f2){rc.out(g[k].x), rc.out(g[k].y)};
        if (q.valid) {
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const int v0 = 32 * c + 8 * qd + 4 * half;
                if (vec_out && v0 + 3 < V) {
                    const unsigned lo = IoBF16::pack2(g[2 * qd].x, g[2 * qd].y);
                    const unsigned hi = IoBF16::pack2(g[2 * qd + 1].x, g[2 * qd + 1].y);
                    *reinterpret_cast<uint2 *>(grow + v0) = make_uint2(lo, hi);
                } else {
                    const float e4[4] = {g[2 * qd].x, g[2 * qd].y, g[2 * qd + 1].x, g[2 * qd + 1].y};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (v0 + e < V) grow[v0 + e] = IoBF16::from_f(e4[e]);
                }
            }
            if (rb >= 0) grow[blank] = IoBF16::from_f(rc.out_blank(gb));
            if (mine) grow[rc.lab] = IoBF16::from_f(rc.out_label(gl));
        }
    });
}

// v summed over the 16 lanes of a DPP row (row_shr 1, 2, 4, 8, lanes shifted in from outside the row read as 0): the
// row's lane 15 holds the total, in one fixed order
__device__ __forceinline__ float dpp_row_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, true));
    return v;
}

// ---------------------------------------------------------------------------------------------------------
// the same passes on the 16x16x32 tile (WTile16): each lane carries two rows (row tiles rt = 0, 1) and 8 of the
// chunk's 32 vocabulary entries of each; the four lane groups g = l >> 4 hold disjoint vocabulary and merge once.
template <int KS, int NB, int NW, class RC>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(2, 2))) void joint_bwd16_kernel(
    DevProblem p, JointArgs j) {
    extern __shared__ __attribute__((aligned(16))) unsigned short wsh[];
    constexpr int K32 = KS / 2;
    if (j.n_dev && (int64_t)blockIdx.x * (32 * NW) >= list_len(j)) {  // past the device count: only its dbias row
        if (j.dbias)
            for (int v = threadIdx.x; v < vpad(p.V); v += blockDim.x)
                j.dbias_part[(int64_t)blockIdx.x * vpad(p.V) + v] = 0.0f;
        return;
    }
    const int lane = threadIdx.x & 63, c16 = lane & 15, g = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * (32 * NW) + (threadIdx.x >> 6) * 32 + c16;
    const RowPos q[2] = {row_pos(p, j, i0), row_pos(p, j, i0 + 16)};
    RC rc[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const RowPos &qr = q[rt];
        const int64_t i = i0 + 16 * rt;
        rc[rt].clear();
        if (qr.valid) {
            rc[rt].stage(p, j, qr);
            if (g == 0 && j.bt_idx) j.bt_idx[i] = (int64_t)qr.b * (j.enc_sb / j.H) + qr.t;
            if (g == 0 && j.bs_idx) j.bs_idx[i] = (int64_t)qr.b * (j.pred_sb / j.H) + qr.s;
        }
    }
    const int V = p.V, blank = p.blank;
    const float *bias = load_bias<KS, NB>(j, V, wsh);
    // dbias: this workgroup's column sums of G, in a fixed order (bitwise reproducible): per chunk, each wave's 32
    // column sums (a DPP row reduction over each lane group's 16 rows) go to that wave's own LDS row (every entry
    // written once), and after the loop the NW rows are added in wave order; the workgroup's row of sums then goes to
    // dbias_part[blockIdx.x] for the ordered sum over workgroups (launch_joint_dbias_sum). launch_tile sizes the LDS.
    const int vp = vpad(V);
    const int wave = threadIdx.x >> 6;
    float *dbw = const_cast<float *>(bias) + vp;  // [NW][vp]
    __syncthreads();  // the bias row in LDS
    bf16x8 bfr[2][K32];
    build_row<K32, 32, true>(j, q[0], 8 * g, i0, bfr[0]);
    build_row<K32, 32, true>(j, q[1], 8 * g, i0 + 16, bfr[1]);

    // exactly 4 vector stores per chunk (2 row tiles x 2 vocabulary tiles) on every wave whose lanes are all valid:
    // leave them in flight at the barrier
    const bool vec_out = (V & 3) == 0;
    const bool leave = vec_out && __ballot(!(q[0].valid && q[1].valid)) == 0;
    unsigned short *grow[2] = {j.G + (q[0].valid ? i0 : 0) * V, j.G + (q[1].valid ? i0 + 16 : 0) * V};
    chunk_loop_with<KS, NB, NW>(
        j, V, wsh, leave ? 4 : -1, [&](const unsigned short *wb) { return WTile16<KS>::template mma<4>(wb, bfr, lane); },
        [&](const typename WTile16<KS>::Acc &acc, int c) {
            const f4 bv[2] = {*reinterpret_cast<const f4 *>(bias + 32 * c + 4 * g),
                              *reinterpret_cast<const f4 *>(bias + 32 * c + 16 + 4 * g)};
            const int jb = blank - 32 * c;
            const bool hb = jb >= 0 && jb < 32 && ((jb >> 2) & 3) == g;
            float cs[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // dbias: this lane's two rows
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                float x[8];
                logits8<KS>(acc, bv, rt, x);
                if constexpr (RC::kHat) {  // the blank logit out of the row before the exp (its chunk only): e = 0 there
                    if (jb >= 0 && jb < 32) {
                        const int kb = hb ? pick8_index(jb) : -1;
#pragma unroll
                        for (int k = 0; k < 8; ++k) x[k] = (k == kb) ? NEG_INF_F : x[k];
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) x[k] = fast_exp2(fmaf(x[k], kLog2e, rc[rt].c2));
                // the <= 2 corrected entries of the row are rewritten by a second (2-byte) store after the vector store
                const int jl = rc[rt].lab - 32 * c;
                const bool mine = rc[rt].lab >= 0 && jl >= 0 && jl < 32 && ((jl >> 2) & 3) == g;
                float gb = 0.0f, gl = 0.0f;
                if (jb >= 0 && jb < 32) gb = pick8(x, pick8_index(jb));
                if (__ballot(mine)) gl = pick8(x, pick8_index(jl & 31));
                if (q[rt].valid) {
#pragma unroll
                    for (int vt = 0; vt < 2; ++vt) {
                        const int v0 = 32 * c + 16 * vt + 4 * g;
                        const float e4[4] = {rc[rt].out(x[4 * vt]), rc[rt].out(x[4 * vt + 1]), rc[rt].out(x[4 * vt + 2]),
                                             rc[rt].out(x[4 * vt + 3])};
#pragma unroll
                        for (int e = 0; e < 4; ++e) cs[4 * vt + e] += e4[e];
                        if (vec_out && v0 + 3 < V) {
                            *reinterpret_cast<uint2 *>(grow[rt] + v0) =
                                make_uint2(IoBF16::pack2(e4[0], e4[1]), IoBF16::pack2(e4[2], e4[3]));
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (v0 + e < V) grow[rt][v0 + e] = IoBF16::from_f(e4[e]);
                        }
                    }
                    if (hb) grow[rt][blank] = IoBF16::from_f(rc[rt].out_blank(gb));
                    if (mine) grow[rt][rc[rt].lab] = IoBF16::from_f(rc[rt].out_label(gl));
                    if (j.dbias) {  // the two corrected entries: the column sums above hold them uncorrected
                        const int kb = hb ? pick8_index(jb) : -1, kl = mine ? pick8_index(jl & 31) : -1;
                        const float db = rc[rt].sum_blank(gb), dl = rc[rt].sum_label();
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            if (k == kb) cs[k] -= db;
                            if (k == kl) cs[k] -= dl;
                        }
                    }
                }
            }
            if (j.dbias) {  // sum the 16 lanes of each lane group (one DPP row: rows of the tile), lane 15 adds to LDS
#pragma unroll
                for (int k = 0; k < 8; ++k) cs[k] = dpp_row_sum(cs[k]);
                if (c16 == 15) {
                    float *row = dbw + wave * vp + 32 * c;
#pragma unroll
                    for (int k = 0; k < 8; ++k) row[16 * (k >> 2) + 4 * g + (k & 3)] = cs[k];
                }
            }
        });
    if (j.dbias) {
        __syncthreads();
        float *row = j.dbias_part + (int64_t)blockIdx.x * vp;
        for (int v = threadIdx.x; v < vp; v += blockDim.x) {
            float t = 0.0f;
#pragma unroll
            for (int w = 0; w < NW; ++w) t += dbw[w * vp + v];
            row[v] = t;
        }
    }
}

// One launch shape: a workgroup of 8 waves per CU (two per SIMD, 256 rows sharing each W chunk), two DMA buffers, a
// 2-deep A-fragment ring. (Measured and removed, DESIGN.md §4a: three buffers, two 4-wave workgroups per CU, deeper
// A-fragment rings, the forward on the 16x16x32 tile, a persistent forward, the pipelined one-wave-per-SIMD forward,
// the bias as the initial accumulator and the label logit as a dot product.)
constexpr int kJointNB = 2, kJointNW = 8, kJointRG = 2;

// MF = the backward's MFMA tile (32: 32x32x16, 16: 16x16x32); the forward runs 32x32x16; RC = the backward's row
// coefficients (LossCoef / PathCoef / HatJointCoef); the forward takes its flavour from RC::kHat (HatJointCoef: the
// factorised-blank epilogue)
template <int KS, int MF, bool BWD, class RC>
static hipError_t launch_tile(const DevProblem &p, const JointArgs &j, hipStream_t stream) {
    constexpr int NB = kJointNB, NW = kJointNW, RG = kJointRG;
    // LDS: the 16x16x32 backward with dbias keeps one row of column sums per wave (8) behind the bias; the forward a
    // bias * log2 e row (JointArgs::opt bit 1) where both rows fit, the unscaled epilogue otherwise
    const size_t row = sizeof(float) * vpad(p.V);
    const size_t tile = sizeof(unsigned short) * WTile<KS>::ELEMS;
    JointArgs jj = j;
    if (!BWD && NB * tile + 2 * row > 160 * 1024) jj.opt &= ~2;
    const size_t bias = row * ((MF == 16 && BWD && j.dbias) ? 1 + NW : (!BWD && (jj.opt & 2)) ? 2 : 1);
    const size_t lds = NB * tile + bias;
    if (j.dbias && !(MF == 16 && BWD)) return hipErrorInvalidValue;
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const int64_t blocks = (j.n + 32 * NW - 1) / (32 * NW);
    if (blocks * 64 * NW > 0xffffffffll) return hipErrorInvalidValue;  // 32-bit dispatch size in work-items
    void (*kern)(DevProblem, JointArgs);
    if constexpr (MF == 16 && BWD) kern = joint_bwd16_kernel<KS, NB, NW, RC>;
    else if constexpr (BWD) kern = joint_bwd_kernel<KS, NB, NW, RG, RC>;
    else if constexpr (RC::kHat) kern = joint_fwd_kernel<KS, NB, NW, RG, false, true>;
    else {
        kern = joint_fwd_kernel<KS, NB, NW, RG>;
        if constexpr (kVariants)
            if (tuning().joint_trace) kern = joint_fwd_kernel<KS, NB, NW, RG, true>;
    }
    if (const hipError_t e = allow_lds(kern, lds); e != hipSuccess) return e;
    kern<<<(int)blocks, 64 * NW, lds, stream>>>(p, jj);
    return hipGetLastError();
}

// The backward's MFMA tile: 16x16x32 for H <= 512 (its epilogue carries no per-row running state, and there the
// 16x16 tile's higher clock pays), 32x32x16 at H = 640 (the 16x16 one spills there: two rows' state per lane beside
// 160 B-operand registers); the development build can force 32x32x16 (joint_bwd_mfma = 32).
template <int KS, bool BWD, class RC>
static hipError_t launch_kb(const DevProblem &p, const JointArgs &j, hipStream_t stream) {
    constexpr int kDefault = KS > 32 ? 32 : BWD ? Tuning{}.joint_bwd_mfma : 32;
    if constexpr (kVariants && KS <= 32 && BWD) {
        if (tuning().joint_bwd_mfma == 32) return launch_tile<KS, 32, BWD, RC>(p, j, stream);
    }
    return launch_tile<KS, kDefault, BWD, RC>(p, j, stream);
}

size_t joint_min_lds_bytes(int H, int V) {  // two weight tiles + the bias row
    return kJointNB * sizeof(unsigned short) * 32 * (size_t)H + sizeof(float) * vpad(V);
}

size_t joint_dbias_lds_bytes(int H, int V) {  // the 16x16x32 backward with dbias: + one column-sum row per wave
    return joint_min_lds_bytes(H, V) + kJointNW * sizeof(float) * vpad(V);
}

// The forward (p.hat: the factorised-blank flavour), or the gradient pass with the row coefficients of `coef`
// (kJointCoef*: LossCoef / PathCoef / HatJointCoef), at hidden size H = 16 KS
template <int KS>
static hipError_t launch_pass(const DevProblem &p, const JointArgs &j, bool bwd, int coef, hipStream_t stream) {
    if (!bwd)
        return p.hat ? launch_kb<KS, false, HatJointCoef>(p, j, stream) : launch_kb<KS, false, LossCoef>(p, j, stream);
    switch (coef) {
        case kJointCoefHat: return launch_kb<KS, true, HatJointCoef>(p, j, stream);
        case kJointCoefPath: return launch_kb<KS, true, PathCoef>(p, j, stream);
        default: return launch_kb<KS, true, LossCoef>(p, j, stream);
    }
}

static hipError_t launch_joint(const DevProblem &p, const JointArgs &j, bool bwd, int coef, hipStream_t stream) {
    if (j.n <= 0) return hipSuccess;
    switch (j.H) {
        case 128: return launch_pass<8>(p, j, bwd, coef, stream);
        case 256: return launch_pass<16>(p, j, bwd, coef, stream);
        case 384: return launch_pass<24>(p, j, bwd, coef, stream);
        case 512: return launch_pass<32>(p, j, bwd, coef, stream);
        case 640: return launch_pass<40>(p, j, bwd, coef, stream);
        default: return hipErrorInvalidValue;
    }
}

// flag = 1 when max_v (sum_h |W[v, h]| + |bias[v]|) <= 64: every logit z = W_v . h + b_v with |h| <= 1 (tanh,
// rounded to bf16) then lies in [-64, 64]. One workgroup (no cross-workgroup combine, no flag reset launch), a wave per
// weight row at a time, 16-byte loads (a 1 KiB row of H = 512 in one load per lane group): the V x H bf16 weights
// (1 MiB at the headline joint size) are read once, a few microseconds. NaN / inf weights compare false: flag 0, the
// running-max epilogue.
__global__ __launch_bounds__(1024) void joint_wbound_kernel(const unsigned short *__restrict__ W,
                                                            const float *__restrict__ bias, int V, int H,
                                                            int *__restrict__ flag) {
    __shared__ int bad;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    int mine = 0;
    for (int v0 = wave; v0 < V; v0 += 64) {  // four rows per wave per pass: eight loads in flight per lane
        float s[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int v = v0 + 16 * r;
            s[r] = 0.0f;
#pragma unroll
            for (int k = 0; k < 2; ++k) {  // H <= 640 < 1024 (the joint plan's shapes), a multiple of 8
                const int h = 8 * lane + 512 * k;
                if (v < V && h < H) {
                    const uint4 u = *reinterpret_cast<const uint4 *>(W + (int64_t)v * H + h);
                    s[r] += (fabsf(bf16_lo(u.x)) + fabsf(bf16_hi(u.x))) + (fabsf(bf16_lo(u.y)) + fabsf(bf16_hi(u.y))) +
                            (fabsf(bf16_lo(u.z)) + fabsf(bf16_hi(u.z))) + (fabsf(bf16_lo(u.w)) + fabsf(bf16_hi(u.w)));
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int v = v0 + 16 * r;
            float t = s[r];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o);
            if (v < V) {
                if (bias) t += fabsf(bias[v]);
                if (!(t <= 64.0f)) mine = 1;
            }
        }
    }
    if (mine && lane == 0) atomicOr(&bad, 1);
    __syncthreads();
    if (threadIdx.x == 0) *flag = bad ? 0 : 1;
}

hipError_t launch_joint_wbound(const unsigned short *W, const float *bias, int V, int H, int *flag,
                               hipStream_t stream) {
    if (V <= 0 || H <= 0 || H > 1024 || (H & 7)) return hipErrorInvalidValue;
    joint_wbound_kernel<<<1, 1024, 0, stream>>>(W, bias, V, H, flag);
    return hipGetLastError();
}

hipError_t launch_joint_forward(const DevProblem &p, const JointArgs &j, hipStream_t stream) {
    JointArgs jp = j;
    if (kVariants && tuning().joint_probe) {
        jp.probe = tuning().joint_probe;
        if (jp.probe & 8) jp.wplain = nullptr;  // (A/B: the running-max epilogue whatever the bound)
    }
    return launch_joint(p, jp, false, kJointCoefLoss, stream);
}

hipError_t launch_joint_backward(const DevProblem &p, const JointArgs &j, hipStream_t stream, int coef) {
    return launch_joint(p, j, true, coef, stream);
}

}  // namespace mrnnt
