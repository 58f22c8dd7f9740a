// mrnnt_host.h -- declarations shared by the host translation units of libmonotonic_rnnt_amd.so: the HIP side
// (hipcc: mrnnt_plan.h and the units that include it), the host-only C ABI (mrnnt_entry.cpp, g++) and the CPU
// implementation (mrnnt_cpu.cpp, g++). Plain C++, no HIP types.
// Not installed; not part of the ABI.
#pragma once

#include <string>

#include "options.h"
#include "status.h"
#include "workspace_manager.h"

namespace mrnnt {

// Record `msg` as this thread's mrnnt_last_error() and return `st` (defined in mrnnt_entry.cpp).
RNNTStatus set_error(RNNTStatus st, const std::string &msg);

// compute_rnnt_loss for loc = RNNT_GPU (mrnnt_manager.cpp; a weak stub in mrnnt_entry.cpp serves host-only builds).
RNNTStatus gpu_compute_rnnt_loss(RNNTWorkspaceManager &workspace_manager, RNNTOptions options, float *costs,
                                 float *gradients);

// A lattice row (t, s) with alpha(t-1, s) + beta(t, s) - ll < kDeadLogOcc has occupancy below e^-110 =
// 2^-158.7: every element of its fp32 gradient, p_v * occupancy minus the blank / label corrections (each
// bounded by the occupancy), is below half the smallest fp32 denormal (2^-150) and rounds to exactly 0 --
// in these kernels and in the reference's fp32 arithmetic alike. Such rows are stored as 0 * grad_scale
// without reading acts. (NaN state compares false and takes the full path.)
constexpr double kDeadLogOcc = -110.0;

// Flush-dead rows of the stored-logits loss gradient (LossRows, mrnnt_grad.hip; tuning occ_skip = 1). The fp32
// kernels are not IEEE below the normal range: every element is fast_exp2(fmaf(z, kLog2e, c2)), the raw v_exp_f32,
// which returns +0 for every argument <= -126 - 2^-6 (measured over every fp32 in [-150, -126] and down to -inf:
// mrnnt_exp2_probe, tests/test_gpu_flush_rows.py; in fact for every argument < -126). A row that is live under
// kDeadLogOcc is flush-dead iff
//     ub + flush_eps_log2(den_f, V) < kFlushLog2,   cb == 0.0f,   ce == 0.0f,
//     ub = (double)c2 + (-(double)den_f) * (double)kLog2e
// with c2, cb, ce the fp32 coefficients the row would be staged with and den_f the stored fp32 denominator (a NaN in
// any of them compares false: the row stays live). Then the row is bit for bit zero_row_value(ll, sc):
//   - z <= -den_f + eps for every element of the row, where den = -max - ln(sum) (write_row / log_row_sum, shared by
//     every log-softmax form) and eps depends on how the form sums:
//       * softmax_kernel (softmax_variant 0 / 2) and the scalar form take exp2((x - max) * kLog2e): the maximum's own
//         term is exactly 1, sum >= 1, and -den >= max up to the error of log_row_sum near 1 (~3e-8) and the fp32
//         rounding of den: eps < 1e-7;
//       * the lean kernel, the 16-lane rows and the chase bodies built from them (producers and self-help) take
//         exp2(fmaf(x, kLog2e, off)) with off = -fl32(max * kLog2e): the maximum's own term is 2^d, d the rounding
//         error of max * kLog2e, |d| <= ulp(max * kLog2e) / 2 <= ulp(max), and it can be below 1. The running-max
//         form rescales its sum by the same 2^d once per further chunk of the row (a chunk is >= 256 elements), so
//         sum >= 2^(n d) for a row of n <= V / 256 + 1 chunks: ln(sum) >= -0.7 n ulp(max) (less n v_exp_f32 errors
//         of ~1.2e-7 relative), and den's own rounding adds at most ulp(max) / 2. So
//             eps <= (0.7 n + 0.5) ulp(max) + n 3e-7,   ulp(max) <= |max| 2^-23,   |max| <= |den_f| + ln(V) + eps:
//         up to a few ulp of the row maximum -- 1e-3 for logits near 1.2e4, 1.6e-2 near 2e5 -- not a constant;
//     f32, bf16 and fp16 acts alike (they are widened exactly). flush_eps_log2 below is at least twice
//     eps * log2(e) for every form; tests/test_gpu_flush_rows.py measures max_v z + den_f against half of it on every
//     form, at logit offsets on either side of a binade of max * kLog2e;
//   - fmaf is one rounding of z * kLog2e + c2, rounding is monotone and kLog2e > 0, so every exp2 argument is at most
//     the fp32 rounding of ub + eps * log2(e) < kFlushLog2, i.e. <= kFlushLog2 (which is an fp32 number); the 2^-6
//     between kFlushLog2 and -126, where the probe shows the flush to begin, is not spent on eps at all;
//   - so every exp2 is +0, the corrections are +0, and each element is (+0 - (+0 + +0)) * sc = +0 * sc: the value and
//     sign zero_row_value(ll, sc) has for a finite ll, for negative, zero, infinite and NaN sc alike. (ll = -inf or NaN
//     makes c2 +inf or NaN: live.)
// Why whole rows qualify: z_v + den <= 0, so the largest argument of a row is at most log2(occupancy), and
// beta(t, s) is at least either of its two terms, so cb's and ce's arguments are too: rows with log-occupancy in
// [-110, -87.34) are flush-dead up to where ln(sum) puts den. Every other user of RowCoef::live keeps
// kDeadLogOcc alone: their element formulas multiply normal numbers, which do keep denormals.
constexpr double kFlushLog2 = -126.015625;  // -126 - 2^-6
// >= 2 eps log2(e) for a row of V elements with stored denominator den: (|den| + 32) (V / 256 + 2) 2^-22. With
// n + 1 <= V / 256 + 2: eps log2(e) <= 1.01 (n + 1) (|den| + 23) 2^-23 + n 4.4e-7 (ln V < 23), half of this or less.
// A NaN den gives NaN (the comparison is false, the row live), an infinite one +inf (live).
constexpr double flush_eps_log2(double den, int V) {
    return ((den < 0.0 ? -den : den) + 32.0) * (double)(V / 256 + 2) * (1.0 / 4194304.0);
}

// The host path's twin (LossRows, mrnnt_cpu.cpp): vexp(x) is exactly 0 for x < -87, x = fl32(z + c) one rounding of
// z + c <= c - den_f + eps (eps = 0 there: vexp(0) = 1 and the fp64 log of a sum >= 1 is >= 0), so every element of a
// row with (double)c - (double)den_f < kFlushLnCpu is +0; the blank / label corrections are IEEE (std::exp, denormals
// kept), and have to be 0 themselves.
constexpr double kFlushLnCpu = -87.015625;  // -87 - 2^-6

}  // namespace mrnnt
