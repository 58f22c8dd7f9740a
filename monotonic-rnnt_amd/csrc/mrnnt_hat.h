// mrnnt_hat.h -- row coefficients of the factorised-blank (HAT) logit gradient, shared by the streaming gradient
// kernels over stored logits (HatRows, mrnnt_hat.hip) and the MFMA gradient kernels of the fused joint (HatJointCoef,
// mrnnt_joint.hip): one definition, so the two paths stage the same values from the same workspace state.
// With the arc posteriors of the row, cb = exp(lpb + alpha(t-1,s) + beta(t+1,s) - ll) and
// ce = exp(lpe + alpha(t-1,s) + beta(t+1,s+1) - ll) (0 at s = S),
//   g[b]      = ce sigmoid(z_b) - cb sigmoid(-z_b)
//   g[v != b] = ce (exp(z_v + den') - [v == label(s)]),   den' = -LSE_{u != b} z_u
#pragma once

#include "mrnnt_device.h"

namespace mrnnt {

struct HatCoef {
    float c2;  // (den' + lpe + alpha(t-1,s) + beta(t+1,s+1) - ll) * log2(e), -inf where ce = 0 (s = S among them):
               // exp2(z log2(e) + c2) = ce softmax_{u != b}(z)
    float ce;  // label-arc posterior
    float gb;  // the blank element: ce sigmoid(z_b) - cb sigmoid(-z_b)
    int lab;   // label(s) (-1 for s == S, label == blank or out of range)
};

// false: the row's gradient is exactly zero in fp32 -- ce and the blank element both are (NaN counts as non-zero)
__device__ __forceinline__ bool hat_coef(const DevProblem &p, int t, int T, int S, int s, int64_t row, double ll,
                                         const int *__restrict__ lab_b, HatCoef &rc) {
    const int W = S + 1;
    const double am = alpha_prev(p, t, s, row, W);
    const double b1 = (t == T - 1) ? (s == S ? 0.0 : NEG_INF_D) : p.beta[row + W];
    const double b2 = (s == S) ? NEG_INF_D : ((t == T - 1) ? (s + 1 == S ? 0.0 : NEG_INF_D) : p.beta[row + W + 1]);
    const double base = am - ll;
    const Lp l = p.lp[row];
    // the exponents are O(10) after the fp64 cancellation of alpha + beta - ll (row_coef, mrnnt_device.h)
    const float cb = fast_exp2((float)((l.b + base + b1) * kLog2eD));
    const double le = l.e + base + b2;
    rc.ce = (s < S) ? fast_exp2((float)(le * kLog2eD)) : 0.0f;
    // (no label arc, ce = 0: every non-blank element is 0 -- also where den' = +inf, a row with every label masked)
    rc.c2 = (s < S && rc.ce != 0.0f) ? (float)(((double)p.den[row] + le) * kLog2eD) : NEG_INF_F;
    // sigmoid(z_b) = exp(lpb); sigmoid(-z_b) = 1 - exp(lpb), as -expm1(lpb) where the difference would cancel
    const float q = (float)l.b;
    const float sp = fast_exp2(q * kLog2e);
    const float sn = q > -0.5f ? -expm1f(q) : 1.0f - sp;
    rc.gb = rc.ce * sp - cb * sn;
    const int lab = (s < S) ? lab_b[s] : -1;
    rc.lab = (lab == p.blank || (unsigned)lab >= (unsigned)p.V) ? -1 : lab;
    return !p.occ_skip || rc.ce != 0.0f || rc.gb != 0.0f;
}

}  // namespace mrnnt
