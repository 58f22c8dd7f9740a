// mrnnt_joint_capi.cpp -- the fused joint network + loss ABI of libmonotonic_rnnt_amd.so (mrnnt_joint_* in
// include/mrnnt.h): the loss plan of mrnnt_plan.h extended by the row lists of the joint kernels (mrnnt_joint_rows.hip;
// mrnnt_joint.hip, mrnnt_joint_reduce.hip, mrnnt_joint_gemm.hip). mrnnt_joint_align / mrnnt_joint_posteriors / mrnnt_joint_sample put the Viterbi launch / the
// posterior read-out / the path sampler of the loss ABI behind the joint's log-softmax pass; mrnnt_joint_path_* score
// given alignments (mrnnt_path.hip's walk / hull / score / coef launches around the joint pass over the hull rows) and
// run the gradient pass over the path-live rows; mrnnt_joint_expect_* put the expectation recursion of
// mrnnt_expect.hip behind the joint forward, form the expected cost's row weights (launch_expect_coef) and run the same
// gradient pass over the expect-live rows; mrnnt_joint_hat_forward / _backward / _align are the factorised-blank (HAT)
// loss on the same plan, workspace and row lists -- thin wrappers over the *_impl functions below with a `hat` flag.
// Asynchronous on the caller's stream, no host synchronisation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#pragma GCC visibility push(default)
#include "mrnnt.h"
#pragma GCC visibility pop
#include "mrnnt_plan.h"

using namespace mrnnt;

namespace {

struct JointPlan {
    Plan base;
    int64_t n_inband = 0;
    size_t off_cnt = 0, off_lcol = 0, off_ls = 0, off_total = 0, off_wplain = 0, off_dbias = 0, total = 0;
};

mrnnt_problem base_problem(const mrnnt_joint_problem *jp) {
    mrnnt_problem p;
    std::memset(&p, 0, sizeof(p));
    p.B = jp->B;
    p.V = jp->V;
    p.blank = jp->blank;
    p.T_host = jp->T_host;
    p.S_host = jp->S_host;
    p.T_dev = jp->T_dev;
    p.S_dev = jp->S_dev;
    p.acts = jp->enc;  // the lattice kernels never read acts on this path
    p.labels = jp->labels;
    p.label_stride = jp->label_stride;
    p.alignment = jp->alignment;
    p.align_stride = jp->align_stride;
    p.align_blank = jp->align_blank;
    p.max_shift = jp->max_shift;
    p.num_rows = -1;
    return p;
}

bool aligned16(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }

RNNTStatus make_joint_plan(const mrnnt_joint_problem *jp, JointPlan *jl) {
    if (!jp) return fail(RNNT_STATUS_INVALID_VALUE, "null joint problem");
    const mrnnt_problem p = base_problem(jp);
    JointPlan q;
    RNNTStatus st = make_plan(&p, &q.base);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const int H = jp->H;
    if (H != 128 && H != 256 && H != 384 && H != 512 && H != 640)
        return fail(RNNT_STATUS_INVALID_VALUE, "joint H must be 128, 256, 384, 512 or 640 (got " + std::to_string(H) + ")");
    if (joint_min_lds_bytes(H, jp->V) > 160 * 1024)
        return fail(RNNT_STATUS_INVALID_VALUE, "V = " + std::to_string(jp->V) + " is too large for the fused joint kernels at H = " +
                                                   std::to_string(H) + " (weight tiles + bias need " +
                                                   std::to_string(joint_min_lds_bytes(H, jp->V) / 1024) +
                                                   " KiB of LDS, 160 KiB per CU); use the unfused loss");
    if (jp->enc_stride % 8 || jp->pred_stride % 8)
        return fail(RNNT_STATUS_INVALID_VALUE, "enc/pred utterance strides must be multiples of 8 elements");
    if (jp->hact_ld != 0 && (jp->hact_ld < H || jp->hact_ld % 8))
        return fail(RNNT_STATUS_INVALID_VALUE, "hact_ld must be 0 or a multiple of 8 that is >= H");
    if (jp->enc_stride < (int64_t)q.base.T_max * H || jp->pred_stride < (int64_t)(q.base.S_max + 1) * H)
        return fail(RNNT_STATUS_INVALID_VALUE, "enc/pred utterance strides smaller than max T * H / (max S + 1) * H");
    for (int b = 0; b < jp->B; ++b) q.n_inband += inband_rows(jp->T_host[b], jp->S_host[b]);
    Carver c{q.base.total};
    // per-column counts + their exclusive scan, and the scan's tile sums (launch_row_list)
    q.off_cnt = c.take(sizeof(int64_t) * (q.base.cols + 2 + (q.base.cols + 1023) / 1024));
    q.off_lcol = c.take(sizeof(int) * std::max<int64_t>(1, q.n_inband));
    q.off_ls = c.take(sizeof(int) * std::max<int64_t>(1, q.n_inband));
    q.off_total = c.take(sizeof(unsigned long long));
    q.off_wplain = c.take(sizeof(int));  // the forward's weight-bound flag (launch_joint_wbound)
    // the gradient pass's per-workgroup dbias column sums (fixed-order reduction), when there is a bias
    q.off_dbias = (jp->bias && H <= 512) ? c.take(joint_dbias_part_bytes(std::max<int64_t>(1, q.n_inband), jp->V)) : 0;
    q.total = c.at;
    *jl = q;
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus check_joint_pointers(const mrnnt_joint_problem *jp) {
    if (!jp->enc || !jp->pred || !jp->weight) return fail(RNNT_STATUS_INVALID_VALUE, "enc / pred / weight is null");
    if (!aligned16(jp->enc) || !aligned16(jp->pred) || !aligned16(jp->weight))
        return fail(RNNT_STATUS_INVALID_VALUE, "enc / pred / weight must be 16-byte aligned");
    if (!jp->T_dev || !jp->S_dev) return fail(RNNT_STATUS_INVALID_VALUE, "device lengths are required");
    if (!jp->labels) return fail(RNNT_STATUS_INVALID_VALUE, "labels is null");
    return RNNT_STATUS_SUCCESS;
}

JointArgs joint_args(const mrnnt_joint_problem *jp, const JointPlan &jl, void *ws, int64_t n) {
    JointArgs j;
    std::memset(&j, 0, sizeof(j));
    j.enc = static_cast<const unsigned short *>(jp->enc);
    j.enc_sb = jp->enc_stride;
    j.pred = static_cast<const unsigned short *>(jp->pred);
    j.pred_sb = jp->pred_stride;
    j.W = static_cast<const unsigned short *>(jp->weight);
    j.bias = jp->bias;
    j.H = jp->H;
    j.hact_ld = jp->hact_ld ? jp->hact_ld : jp->H;
    j.lcol = carve<int>(ws, jl.off_lcol);
    j.ls = carve<int>(ws, jl.off_ls);
    j.n = n;
    j.opt = kVariants ? tuning().joint_opt : 3;
    return j;
}

// The joint forward pass over the rows d's band lets through (the row list in mode 0): lpb / lpe and den of each into
// the workspace. windowed: the band is narrower than the monotonic one, the number of rows stays on the device.
RNNTStatus joint_forward_pass(const mrnnt_joint_problem *jp, const JointPlan &jl, void *ws, const DevProblem &d,
                              bool windowed, hipStream_t stream) {
    unsigned long long *total = carve<unsigned long long>(ws, jl.off_total);
    hipError_t e = launch_row_list(d, 0, carve<int64_t>(ws, jl.off_cnt), carve<int>(ws, jl.off_lcol),
                                   carve<int>(ws, jl.off_ls), total, stream);
    if (e != hipSuccess) return fail_hip(e, "row list kernels");
    JointArgs j = joint_args(jp, jl, ws, jl.n_inband);
    if (windowed) j.n_dev = total;
    // the weight bound decides the forward's epilogue on the device (no host sync): counted in the forward's time
    int *wplain = carve<int>(ws, jl.off_wplain);
    j.wplain = wplain;
    e = timed(K_JOINT_FWD, stream, [&] {
        const hipError_t eb = launch_joint_wbound(j.W, j.bias, jp->V, jp->H, wplain, stream);
        return eb != hipSuccess ? eb : launch_joint_forward(d, j, stream);
    });
    if (e != hipSuccess) return fail_hip(e, "joint log-softmax kernel");
    return RNNT_STATUS_SUCCESS;
}

// What mrnnt_joint_forward and mrnnt_joint_align share after the plan: pointer and workspace checks, the lattice (and
// the alignment band), then the joint log-softmax pass that leaves lpb / lpe of every row the recursion can use in the
// workspace. *out: the device problem for the launch that follows (launch_dp / launch_viterbi). hat: the
// factorised-blank flavour of the joint pass (DevProblem::hat): den' and hat_lp's pair in the same arrays.
RNNTStatus joint_log_softmax(const mrnnt_joint_problem *jp, const JointPlan &jl, void *ws, size_t ws_bytes,
                             int64_t t_cap, hipStream_t stream, DevProblem *out, bool hat = false) {
    RNNTStatus st = check_joint_pointers(jp);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_workspace(ws, ws_bytes, jl.total)) != RNNT_STATUS_SUCCESS) return st;
    const Plan &pl = jl.base;
    const mrnnt_problem p = base_problem(jp);  // host lengths, no caller lattice: the setup kernel builds the offsets
    DevProblem d = make_dev(&p, pl, ws);
    d.hat = hat ? 1 : 0;
    LatticeOpts o;
    o.t_cap = t_cap;
    if ((st = prepare_lattice(&p, pl, d, ws, o, stream)) != RNNT_STATUS_SUCCESS) return st;
    // out-of-band lp entries must be finite for the recursion (the acts path zero-fills them in its pass)
    hipError_t e = launch_zero(carve<char>(ws, pl.off_lp), pl.off_alpha - pl.off_lp, stream);
    if (e != hipSuccess) return fail_hip(e, "lp zero fill");
    if ((st = joint_forward_pass(jp, jl, ws, d, pl.align, stream)) != RNNT_STATUS_SUCCESS) return st;  // alignment windows
    *out = d;
    return RNNT_STATUS_SUCCESS;
}

// mrnnt_joint_path_*: the ordinary joint workspace of the same problem (make_joint_plan of jp, which has no alignment),
// FOLLOWED by the band arrays (the hull of the paths) and the per-path words. mrnnt_joint_reduce / _reduce_pre / _dpre
// rebuild the ordinary plan from jp and carve the workspace by its offsets: they work on this one unchanged.
struct JointPathPlan {
    JointPlan jl;
    int64_t row_bound = 0;  // sum_b min(num_paths * T_b, in-band rows of b) >= the path-live rows
    size_t off_min = 0, off_max = 0, off_valid = 0, off_carry = 0, total = 0;
};

// The plan and the host checks of the joint path entry points, all before any device call (make_path_plan's).
RNNTStatus make_joint_path_plan(const mrnnt_joint_problem *jp, int num_paths, JointPathPlan *pp) {
    const Plan &pl = pp->jl.base;
    const RNNTStatus st =
        plan_paths(jp && jp->alignment, num_paths, pl, [&] { return make_joint_plan(jp, &pp->jl); });
    if (st != RNNT_STATUS_SUCCESS) return st;
    pp->row_bound = 0;
    for (int b = 0; b < jp->B; ++b)
        pp->row_bound += std::min<int64_t>((int64_t)num_paths * jp->T_host[b], inband_rows(jp->T_host[b], jp->S_host[b]));
    Carver c{pp->jl.total};
    pp->off_min = c.take(sizeof(int) * (size_t)pl.cols);
    pp->off_max = c.take(sizeof(int) * (size_t)pl.cols);
    pp->off_valid = c.take(sizeof(int) * (size_t)pl.B * num_paths);
    pp->off_carry = c.take(sizeof(int) * (size_t)path_carry_slots(pl.cols, pl.B) * num_paths);
    pp->total = c.at;
    return RNNT_STATUS_SUCCESS;
}

// the device problem with the hull as its band, and the path words
DevProblem joint_path_dev(const mrnnt_problem *p, const JointPathPlan &pp, void *ws) {
    DevProblem d = make_dev(p, pp.jl.base, ws);
    d.min_s = carve<int>(ws, pp.off_min);
    d.max_s = carve<int>(ws, pp.off_max);
    return d;
}

PathArgs joint_path_args(const JointPathPlan &pp, void *ws, const int *alignments_dev, int num_paths,
                         int64_t path_stride) {
    return path_args(ws, pp.off_valid, pp.off_carry, pp.off_min, pp.off_max, alignments_dev, num_paths, path_stride);
}

// mrnnt_joint_expect_*: the ordinary joint workspace of the same problem (a restricting alignment included), FOLLOWED
// by the expectation state A / Bk (fp64 [N]) and R (fp64 [B]) and the two row-weight arrays Wb / We (fp64 [N]) of the
// coefficient launch. mrnnt_joint_reduce / _reduce_pre / _dpre work on it unchanged, as on the path workspace.
struct JointExpectPlan {
    JointPlan jl;
    ExpectState state;
    size_t off_wb = 0, off_we = 0, total = 0;
};

RNNTStatus make_joint_expect_plan(const mrnnt_joint_problem *jp, JointExpectPlan *ep) {
    const RNNTStatus st = make_joint_plan(jp, &ep->jl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const Plan &pl = ep->jl.base;
    Carver c{ep->jl.total};
    ep->state.carve_from(&c, pl);
    ep->off_wb = c.take(sizeof(double) * (size_t)pl.N);
    ep->off_we = c.take(sizeof(double) * (size_t)pl.N);
    ep->total = c.at;
    return RNNT_STATUS_SUCCESS;
}

// The device problem of the expectation launches: the packed lattice of the joint, the state arrays, and the cost
// arrays on the caller's grid -- only acts_col_base, which the expectation kernels address the costs through, takes
// the padded mapping (as mrnnt_joint_posteriors' outputs do).
DevProblem joint_expect_dev(const mrnnt_problem *p, const JointExpectPlan &ep, void *ws, const float *blank_cost_dev,
                            const float *label_cost_dev, int64_t grid_T, int64_t grid_S1) {
    DevProblem d = make_dev(p, ep.jl.base, ws);
    ep.state.bind(&d, ws, blank_cost_dev, label_cost_dev);
    if (blank_cost_dev || label_cost_dev) {
        d.pad_T = grid_T;
        d.pad_S1 = grid_S1;
    }
    return d;
}

// mrnnt_joint_backward / mrnnt_joint_path_backward / mrnnt_joint_expect_backward: the MFMA gradient pass over the rows
// of the last list built, with the loss's row coefficients (alpha / beta / ll, times scale), the path weights (path:
// Wb / We in alpha / beta) or the expected cost's (expect: the path coefficients on a device problem whose alpha / beta
// point at the coefficient launch's Wb / We arrays -- the same kernel instantiation) or the factorised-blank loss's
// (hat: hat_coef over the state of mrnnt_joint_hat_forward).
enum JointCoef { kCoefLoss, kCoefPath, kCoefExpect, kCoefHat };

RNNTStatus joint_backward(const mrnnt_joint_problem *jp, void *ws, int64_t n_live, const float *grad_scale, void *G,
                          void *Hact, int64_t *bt_idx, int64_t *bs_idx, JointCoef coef, hipStream_t stream) {
    const bool path = coef == kCoefPath;
    JointExpectPlan ep;
    RNNTStatus st = make_joint_expect_plan(jp, &ep);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const JointPlan &jl = ep.jl;
    if (path && jp->alignment)
        return fail(RNNT_STATUS_INVALID_VALUE, "path scores take no restricting alignment (p->alignment must be NULL)");
    if ((st = check_joint_pointers(jp)) != RNNT_STATUS_SUCCESS) return st;
    if (!ws) return fail(RNNT_STATUS_INVALID_VALUE, "workspace is null");
    if (n_live < 0 || n_live > jl.n_inband)
        return fail(RNNT_STATUS_INVALID_VALUE, "n_live outside [0, in-band rows]");
    if (n_live > 0 && (!G || !Hact)) return fail(RNNT_STATUS_INVALID_VALUE, "G / Hact is null");
    if (n_live > 0 && (!aligned16(G) || !aligned16(Hact)))
        return fail(RNNT_STATUS_INVALID_VALUE, "G / Hact must be 16-byte aligned");
    const mrnnt_problem p = base_problem(jp);
    DevProblem d = make_dev(&p, jl.base, ws);
    if (coef == kCoefExpect) {
        d.alpha = carve<double>(ws, ep.off_wb);
        d.beta = carve<double>(ws, ep.off_we);
    }
    JointArgs j = joint_args(jp, jl, ws, n_live);
    j.n_dev = jp->live_count_dev;  // n_live a host bound: workgroups past the device count exit (their rows zeroed below)
    j.G = static_cast<unsigned short *>(G);
    j.Hact = static_cast<unsigned short *>(Hact);
    j.bt_idx = bt_idx;
    j.bs_idx = bs_idx;
    j.scale = grad_scale;
    j.dbias = jp->dbias;
    if (jp->dbias && jp->H > 512) return fail(RNNT_STATUS_INVALID_VALUE, "dbias in the gradient pass needs H <= 512");
    if (jp->dbias && joint_dbias_lds_bytes(jp->H, jp->V) > 160 * 1024)
        return fail(RNNT_STATUS_INVALID_VALUE, "dbias in the gradient pass: V too large for its LDS column sums at this H "
                                               "(sum G's columns outside: dbias = NULL)");
    if (jp->dbias && !jl.off_dbias)
        return fail(RNNT_STATUS_INVALID_VALUE, "dbias needs a bias (the workspace holds its partial sums only then)");
    if (jp->dbias) j.dbias_part = carve<float>(ws, jl.off_dbias);
    hipError_t e = timed(K_JOINT_BWD, stream, [&] {
        const hipError_t eb = launch_joint_backward(
            d, j, stream, coef == kCoefLoss ? kJointCoefLoss : coef == kCoefHat ? kJointCoefHat : kJointCoefPath);
        if (eb != hipSuccess || !jp->live_count_dev) return eb;
        return launch_joint_tail_zero(j.G, jp->V, j.Hact, j.hact_ld, n_live, jp->live_count_dev, stream);
    });
    if (e != hipSuccess) return fail_hip(e, "joint gradient kernel");
    if (jp->dbias && n_live > 0) {
        e = launch_joint_dbias_sum(j, jp->V, stream);
        if (e != hipSuccess) return fail_hip(e, "joint dbias sum kernels");
    }
    return RNNT_STATUS_SUCCESS;
}

// mrnnt_joint_forward / mrnnt_joint_hat_forward
RNNTStatus joint_forward_impl(const mrnnt_joint_problem *jp, void *ws, size_t ws_bytes, float *costs_dev, int with_beta,
                              hipStream_t stream, bool hat) {
    JointPlan jl;
    RNNTStatus st = make_joint_plan(jp, &jl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    DevProblem d;
    if ((st = joint_log_softmax(jp, jl, ws, ws_bytes, 0, stream, &d, hat)) != RNNT_STATUS_SUCCESS) return st;
    const hipError_t e =
        timed(K_DP, stream, [&] { return launch_dp(d, jl.base.S_max, with_beta ? 1 : 0, costs_dev, stream); });
    if (e != hipSuccess) return fail_hip(e, "alpha/beta kernel");
    return RNNT_STATUS_SUCCESS;
}

// mrnnt_joint_align / mrnnt_joint_hat_align
RNNTStatus joint_align_impl(const mrnnt_joint_problem *jp, void *ws, size_t ws_bytes, int *alignment_out_dev,
                            int64_t out_stride, float *costs_dev, hipStream_t stream, bool hat) {
    JointPlan jl;
    RNNTStatus st = make_joint_plan(jp, &jl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (!alignment_out_dev) return fail(RNNT_STATUS_INVALID_VALUE, "alignment_out is null");
    if ((st = check_row_stride("alignment_out", out_stride, "input", jl.base.T_max, false, 0)) != RNNT_STATUS_SUCCESS)
        return st;
    DevProblem d;
    if ((st = joint_log_softmax(jp, jl, ws, ws_bytes, out_stride, stream, &d, hat)) != RNNT_STATUS_SUCCESS) return st;
    // jp->alignment may be alignment_out_dev itself: the band kernels have consumed it (stream order), the joint
    // pass and the Viterbi launch read only the band arrays
    const hipError_t e = timed(K_DP, stream, [&] {
        return launch_viterbi(d, jl.base.S_max, alignment_out_dev, out_stride, costs_dev, stream);
    });
    if (e != hipSuccess) return fail_hip(e, "viterbi kernel");
    return RNNT_STATUS_SUCCESS;
}

}  // namespace

extern "C" {

RNNTStatus mrnnt_joint_workspace_size(const mrnnt_joint_problem *jp, size_t *bytes) {
    return plan_total<JointPlan>(bytes, [&](JointPlan *jl) { return make_joint_plan(jp, jl); });
}

RNNTStatus mrnnt_joint_row_bound(const mrnnt_joint_problem *jp, int64_t *rows) {
    if (!rows) return fail(RNNT_STATUS_INVALID_VALUE, "null rows pointer");
    JointPlan jl;
    const RNNTStatus st = make_joint_plan(jp, &jl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    *rows = jl.n_inband;
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_joint_forward(const mrnnt_joint_problem *jp, void *ws, size_t ws_bytes, float *costs_dev,
                               int with_beta, hipStream_t stream) {
    return joint_forward_impl(jp, ws, ws_bytes, costs_dev, with_beta, stream, false);
}

RNNTStatus mrnnt_joint_hat_forward(const mrnnt_joint_problem *jp, void *ws, size_t ws_bytes, float *costs_dev,
                                   int with_beta, hipStream_t stream) {
    return joint_forward_impl(jp, ws, ws_bytes, costs_dev, with_beta, stream, true);
}

RNNTStatus mrnnt_joint_align(const mrnnt_joint_problem *jp, void *ws, size_t ws_bytes, int *alignment_out_dev,
                             int64_t out_stride, float *costs_dev, hipStream_t stream) {
    return joint_align_impl(jp, ws, ws_bytes, alignment_out_dev, out_stride, costs_dev, stream, false);
}

RNNTStatus mrnnt_joint_hat_align(const mrnnt_joint_problem *jp, void *ws, size_t ws_bytes, int *alignment_out_dev,
                                 int64_t out_stride, float *costs_dev, hipStream_t stream) {
    return joint_align_impl(jp, ws, ws_bytes, alignment_out_dev, out_stride, costs_dev, stream, true);
}

RNNTStatus mrnnt_joint_posteriors(const mrnnt_joint_problem *jp, const void *ws, float *blank_post_dev,
                                  float *label_post_dev, int64_t grid_T, int64_t grid_S1, float *emit_dev,
                                  int64_t emit_stride, float *label_time_dev, int64_t time_stride, hipStream_t stream) {
    JointPlan jl;
    RNNTStatus st = make_joint_plan(jp, &jl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const Plan &pl = jl.base;
    if ((st = check_grid(pl, blank_post_dev || label_post_dev, "posterior", grid_T, grid_S1)) != RNNT_STATUS_SUCCESS)
        return st;
    if (emit_dev && (st = check_row_stride("emit", emit_stride, "input", pl.T_max, false, 0)) != RNNT_STATUS_SUCCESS)
        return st;
    if (label_time_dev &&
        (st = check_row_stride("label_time", time_stride, "label", pl.S_max, false, 0)) != RNNT_STATUS_SUCCESS)
        return st;
    if (!ws) return fail(RNNT_STATUS_INVALID_VALUE, "workspace is null");
    if (!jp->T_dev || !jp->S_dev) return fail(RNNT_STATUS_INVALID_VALUE, "device lengths are required");
    const mrnnt_problem p = base_problem(jp);
    DevProblem d = make_dev(&p, pl, ws);
    // the lattice is packed (state rows row_off[b] + t * (S_b + 1) + s); only the per-row OUTPUTS take the padded
    // mapping, which the posterior launch keeps apart from the state rows (acts_col_base and its padding fills)
    if (blank_post_dev || label_post_dev) {
        d.pad_T = grid_T;
        d.pad_S1 = grid_S1;
    }
    return posterior_readout(pl, d, {blank_post_dev, label_post_dev, emit_dev, emit_stride, label_time_dev, time_stride},
                             stream);
}

RNNTStatus mrnnt_joint_sample(const mrnnt_joint_problem *jp, const void *ws, int num_samples, uint64_t seed,
                              int64_t first_sample, int *alignments_dev, int64_t out_stride, float *path_costs_dev,
                              hipStream_t stream) {
    JointPlan jl;
    const RNNTStatus st = make_joint_plan(jp, &jl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    // the joint plans its lattice packed and the outputs are [B, K, out_stride]: mrnnt_sample's launch as it is
    const mrnnt_problem p = base_problem(jp);
    return sample_readout(&p, jl.base, ws, num_samples, seed, first_sample, alignments_dev, out_stride, path_costs_dev,
                          stream);
}

RNNTStatus mrnnt_joint_live_rows(const mrnnt_joint_problem *jp, void *ws, unsigned long long *count_dev,
                                 hipStream_t stream) {
    JointPlan jl;
    RNNTStatus st = make_joint_plan(jp, &jl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (!ws || !count_dev) return fail(RNNT_STATUS_INVALID_VALUE, "workspace / count is null");
    const mrnnt_problem p = base_problem(jp);
    DevProblem d = make_dev(&p, jl.base, ws);
    const hipError_t e = launch_row_list(d, 1, carve<int64_t>(ws, jl.off_cnt), carve<int>(ws, jl.off_lcol),
                                         carve<int>(ws, jl.off_ls), count_dev, stream);
    if (e != hipSuccess) return fail_hip(e, "live row list kernels");
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_joint_backward(const mrnnt_joint_problem *jp, void *ws, int64_t n_live, const float *grad_scale,
                                void *G, void *Hact, int64_t *bt_idx, int64_t *bs_idx, hipStream_t stream) {
    return joint_backward(jp, ws, n_live, grad_scale, G, Hact, bt_idx, bs_idx, kCoefLoss, stream);
}

RNNTStatus mrnnt_joint_hat_backward(const mrnnt_joint_problem *jp, void *ws, int64_t n_live, const float *grad_scale,
                                    void *G, void *Hact, int64_t *bt_idx, int64_t *bs_idx, hipStream_t stream) {
    return joint_backward(jp, ws, n_live, grad_scale, G, Hact, bt_idx, bs_idx, kCoefHat, stream);
}

RNNTStatus mrnnt_joint_path_workspace_size(const mrnnt_joint_problem *jp, int num_paths, size_t *bytes) {
    return plan_total<JointPathPlan>(bytes, [&](JointPathPlan *pp) { return make_joint_path_plan(jp, num_paths, pp); });
}

RNNTStatus mrnnt_joint_path_row_bound(const mrnnt_joint_problem *jp, int num_paths, int64_t *rows) {
    if (!rows) return fail(RNNT_STATUS_INVALID_VALUE, "null rows pointer");
    JointPathPlan pp;
    const RNNTStatus st = make_joint_path_plan(jp, num_paths, &pp);
    if (st != RNNT_STATUS_SUCCESS) return st;
    *rows = pp.row_bound;
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_joint_path_forward(const mrnnt_joint_problem *jp, void *ws, size_t ws_bytes, const int *alignments_dev,
                                    int num_paths, int64_t path_stride, float *path_costs_dev, hipStream_t stream) {
    JointPathPlan pp;
    RNNTStatus st = make_joint_path_plan(jp, num_paths, &pp);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const JointPlan &jl = pp.jl;
    const Plan &pl = jl.base;
    if ((st = check_paths(pl, alignments_dev, path_stride)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_joint_pointers(jp)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_workspace(ws, ws_bytes, pp.total)) != RNNT_STATUS_SUCCESS) return st;
    const mrnnt_problem p = base_problem(jp);
    DevProblem d = joint_path_dev(&p, pp, ws);  // d.min_s / d.max_s: the hull
    LatticeOpts o;
    o.t_cap = path_stride;
    if ((st = prepare_lattice(&p, pl, d, ws, o, stream)) != RNNT_STATUS_SUCCESS) return st;
    PathArgs a = joint_path_args(pp, ws, alignments_dev, num_paths, path_stride);
    a.costs = path_costs_dev;
    hipError_t e = timed(K_DP, stream, [&] { return launch_path_walk(d, a, pl.T_max, stream); });
    if (e != hipSuccess) return fail_hip(e, "path walk kernels");
    // the hull rows, listed through the alignment window (mode 0); their number stays on the device. No lp zero fill:
    // no recursion runs, and the score kernel reads lp along the valid walks only -- rows of the hull
    if ((st = joint_forward_pass(jp, jl, ws, d, true, stream)) != RNNT_STATUS_SUCCESS) return st;
    if (path_costs_dev) {
        e = timed(K_DP, stream, [&] { return launch_path_score(d, a, stream); });
        if (e != hipSuccess) return fail_hip(e, "path score kernel");
    }
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_joint_path_rows(const mrnnt_joint_problem *jp, void *ws, size_t ws_bytes, const int *alignments_dev,
                                 int num_paths, int64_t path_stride, const float *weights_dev,
                                 unsigned long long *count_dev, hipStream_t stream) {
    JointPathPlan pp;
    RNNTStatus st = make_joint_path_plan(jp, num_paths, &pp);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const JointPlan &jl = pp.jl;
    if ((st = check_paths(jl.base, alignments_dev, path_stride)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_joint_pointers(jp)) != RNNT_STATUS_SUCCESS) return st;
    if (!count_dev) return fail(RNNT_STATUS_INVALID_VALUE, "count is null");
    if ((st = check_workspace(ws, ws_bytes, pp.total)) != RNNT_STATUS_SUCCESS) return st;
    const mrnnt_problem p = base_problem(jp);
    DevProblem d = joint_path_dev(&p, pp, ws);
    PathArgs a = joint_path_args(pp, ws, alignments_dev, num_paths, path_stride);
    a.w = weights_dev;
    hipError_t e = timed(K_DP, stream, [&] { return launch_path_coef(d, a, jl.base.T_max, stream); });
    if (e != hipSuccess) return fail_hip(e, "path coefficient kernel");
    e = launch_row_list(d, 2, carve<int64_t>(ws, jl.off_cnt), carve<int>(ws, jl.off_lcol), carve<int>(ws, jl.off_ls),
                        count_dev, stream);
    if (e != hipSuccess) return fail_hip(e, "path-live row list kernels");
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_joint_path_backward(const mrnnt_joint_problem *jp, void *ws, int64_t n_rows, void *G, void *Hact,
                                     int64_t *bt_idx, int64_t *bs_idx, hipStream_t stream) {
    return joint_backward(jp, ws, n_rows, nullptr, G, Hact, bt_idx, bs_idx, kCoefPath, stream);
}

RNNTStatus mrnnt_joint_expect_workspace_size(const mrnnt_joint_problem *jp, size_t *bytes) {
    return plan_total<JointExpectPlan>(bytes, [&](JointExpectPlan *ep) { return make_joint_expect_plan(jp, ep); });
}

RNNTStatus mrnnt_joint_expect_forward(const mrnnt_joint_problem *jp, void *ws, size_t ws_bytes,
                                      const float *blank_cost_dev, const float *label_cost_dev, int64_t grid_T,
                                      int64_t grid_S1, float *expected_dev, float *costs_dev, int with_grad,
                                      hipStream_t stream) {
    JointExpectPlan ep;
    RNNTStatus st = make_joint_expect_plan(jp, &ep);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const Plan &pl = ep.jl.base;
    if ((st = check_grid(pl, blank_cost_dev || label_cost_dev, "cost", grid_T, grid_S1)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_joint_pointers(jp)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_workspace(ws, ws_bytes, ep.total)) != RNNT_STATUS_SUCCESS) return st;
    // the joint's forward on the head of the workspace (its own plan: the same offsets), beta only for a gradient
    if ((st = mrnnt_joint_forward(jp, ws, ws_bytes, costs_dev, with_grad ? 1 : 0, stream)) != RNNT_STATUS_SUCCESS)
        return st;
    const mrnnt_problem p = base_problem(jp);
    const DevProblem d = joint_expect_dev(&p, ep, ws, blank_cost_dev, label_cost_dev, grid_T, grid_S1);
    const hipError_t e =
        timed(K_DP, stream, [&] { return launch_expect(d, pl.S_max, with_grad ? 1 : 0, expected_dev, stream); });
    if (e != hipSuccess) return fail_hip(e, "expectation recursion kernel");
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_joint_expect_rows(const mrnnt_joint_problem *jp, void *ws, size_t ws_bytes,
                                   const float *blank_cost_dev, const float *label_cost_dev, int64_t grid_T,
                                   int64_t grid_S1, const float *grad_expected_dev, const float *grad_costs_dev,
                                   unsigned long long *count_dev, hipStream_t stream) {
    JointExpectPlan ep;
    RNNTStatus st = make_joint_expect_plan(jp, &ep);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const JointPlan &jl = ep.jl;
    if ((st = check_grid(jl.base, blank_cost_dev || label_cost_dev, "cost", grid_T, grid_S1)) != RNNT_STATUS_SUCCESS)
        return st;
    if (!count_dev) return fail(RNNT_STATUS_INVALID_VALUE, "count is null");
    if ((st = check_joint_pointers(jp)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_workspace(ws, ws_bytes, ep.total)) != RNNT_STATUS_SUCCESS) return st;
    const mrnnt_problem p = base_problem(jp);
    DevProblem d = joint_expect_dev(&p, ep, ws, blank_cost_dev, label_cost_dev, grid_T, grid_S1);
    d.ex_ge = grad_expected_dev;
    d.ex_gc = grad_costs_dev;
    double *wb = carve<double>(ws, ep.off_wb), *we = carve<double>(ws, ep.off_we);
    hipError_t e = timed(K_DP, stream, [&] { return launch_expect_coef(d, wb, we, stream); });
    if (e != hipSuccess) return fail_hip(e, "expected-cost coefficient kernel");
    d.alpha = wb;  // the list's (and the gradient pass's) view: the two weights where the path scores keep theirs
    d.beta = we;
    e = launch_row_list(d, 3, carve<int64_t>(ws, jl.off_cnt), carve<int>(ws, jl.off_lcol), carve<int>(ws, jl.off_ls),
                        count_dev, stream);
    if (e != hipSuccess) return fail_hip(e, "expect-live row list kernels");
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_joint_expect_backward(const mrnnt_joint_problem *jp, void *ws, int64_t n_rows, void *G, void *Hact,
                                       int64_t *bt_idx, int64_t *bs_idx, hipStream_t stream) {
    return joint_backward(jp, ws, n_rows, nullptr, G, Hact, bt_idx, bs_idx, kCoefExpect, stream);
}

// pre: dH already holds dpre (Hact unused; the kRedPre kernel form)
static RNNTStatus joint_reduce(const mrnnt_joint_problem *jp, void *ws, int64_t n_live, const void *dH,
                               const void *Hact, bool pre, float *d_enc, float *d_pred, hipStream_t stream) {
    JointPlan jl;
    RNNTStatus st = make_joint_plan(jp, &jl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_joint_pointers(jp)) != RNNT_STATUS_SUCCESS) return st;
    if (!ws || !d_enc || !d_pred) return fail(RNNT_STATUS_INVALID_VALUE, "workspace / d_enc / d_pred is null");
    if (n_live < 0 || n_live > jl.n_inband) return fail(RNNT_STATUS_INVALID_VALUE, "n_live outside [0, in-band rows]");
    if (n_live > 0 && (!dH || (reinterpret_cast<uintptr_t>(dH) & 7)))
        return fail(RNNT_STATUS_INVALID_VALUE, pre ? "dpre null or not 8-byte aligned" : "dH null or not 8-byte aligned");
    if (!pre && n_live > 0 && (!Hact || (reinterpret_cast<uintptr_t>(Hact) & 7)))
        return fail(RNNT_STATUS_INVALID_VALUE, "Hact null or not 8-byte aligned (a dH that already holds dpre: "
                                               "mrnnt_joint_reduce_pre)");
    const mrnnt_problem p = base_problem(jp);
    DevProblem d = make_dev(&p, jl.base, ws);
    JointArgs j = joint_args(jp, jl, ws, n_live);
    j.Hact = pre ? nullptr : static_cast<unsigned short *>(const_cast<void *>(Hact));
    const int64_t *off = carve<int64_t>(ws, jl.off_cnt);
    const hipError_t e = timed(K_JOINT_RED, stream, [&] {
        return launch_joint_reduce(d, j, off, jl.base.T_max, jl.base.S_max, static_cast<const unsigned short *>(dH),
                                   d_enc, d_pred, jp->reduce_scratch, jp->reduce_scratch_bytes, stream);
    });
    if (e != hipSuccess) return fail_hip(e, "joint reduce kernel");
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_joint_reduce(const mrnnt_joint_problem *jp, void *ws, int64_t n_live, const void *dH,
                              const void *Hact, float *d_enc, float *d_pred, hipStream_t stream) {
    return joint_reduce(jp, ws, n_live, dH, Hact, false, d_enc, d_pred, stream);
}

RNNTStatus mrnnt_joint_reduce_pre(const mrnnt_joint_problem *jp, void *ws, int64_t n_live, const void *dpre,
                                  float *d_enc, float *d_pred, hipStream_t stream) {
    return joint_reduce(jp, ws, n_live, dpre, nullptr, true, d_enc, d_pred, stream);
}

RNNTStatus mrnnt_joint_dpre(const mrnnt_joint_problem *jp, int64_t n_live, const void *G, const void *weight_t,
                            const void *Hact, void *dpre, hipStream_t stream) {
    JointPlan jl;
    RNNTStatus st = make_joint_plan(jp, &jl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (jp->H != 256 && jp->H != 512)
        return fail(RNNT_STATUS_INVALID_VALUE, "mrnnt_joint_dpre: H must be 256 or 512 (use a library GEMM)");
    if (jp->V % 8) return fail(RNNT_STATUS_INVALID_VALUE, "mrnnt_joint_dpre: V must be a multiple of 8");
    if (n_live < 0 || n_live > jl.n_inband) return fail(RNNT_STATUS_INVALID_VALUE, "n_live outside [0, in-band rows]");
    const int64_t ld = jp->hact_ld ? jp->hact_ld : jp->H;
    if (ld < jp->H || ld % 4) return fail(RNNT_STATUS_INVALID_VALUE, "hact_ld must be >= H and a multiple of 4");
    if (n_live == 0) return RNNT_STATUS_SUCCESS;
    for (const void *q : {G, weight_t, Hact, static_cast<const void *>(dpre)})
        if (!q || (reinterpret_cast<uintptr_t>(q) & 15))
            return fail(RNNT_STATUS_INVALID_VALUE, "mrnnt_joint_dpre: G / weight_t / Hact / dpre null or not 16-byte aligned");
    const hipError_t e = timed(K_JOINT_DPRE, stream, [&] {
        return launch_joint_dpre(static_cast<const unsigned short *>(G), static_cast<const unsigned short *>(weight_t),
                                 static_cast<const unsigned short *>(Hact), ld, static_cast<unsigned short *>(dpre),
                                 n_live, jp->V, jp->H, stream);
    });
    if (e != hipSuccess) return fail_hip(e, "joint dpre kernel");
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_joint_reduce_scratch_bytes(const mrnnt_joint_problem *jp, size_t *bytes) {
    if (!bytes) return fail(RNNT_STATUS_INVALID_VALUE, "null size pointer");
    JointPlan jl;
    const RNNTStatus st = make_joint_plan(jp, &jl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    *bytes = joint_reduce_scratch_bytes(jl.base.B, jl.base.T_max, jl.base.S_max, jp->H);
    return RNNT_STATUS_SUCCESS;
}

}  // extern "C"
