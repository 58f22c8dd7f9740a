// mrnnt_capi.cpp -- the flat loss ABI of libmonotonic_rnnt_amd.so (include/mrnnt.h): each entry point validates,
// plans (mrnnt_plan.h) and launches on the caller's stream. The fused-joint ABI is mrnnt_joint_capi.cpp, the
// reference-shaped C++ surface mrnnt_manager.cpp, the profile entry points mrnnt_plan.cpp.
//
// No host synchronisation happens inside mrnnt_forward / mrnnt_backward (the reference synchronises
// after each reduce and copies T/S/band arrays to the host every call: reduce.h:162,
// gpu_rnnt.h:28-35). The only sync is in the reference-compatible compute_rnnt_loss /
// GpuRNNTComputer path, whose contract returns host costs (gpu_rnnt.h:229).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

// The library is built with -fvisibility=hidden: only the declarations of the public header below are
// exported (the kernels and launchers in mrnnt_internal.h and the shared host code in mrnnt_plan.h stay internal).
#pragma GCC visibility push(default)
#include "mrnnt.h"
#pragma GCC visibility pop
#include "mrnnt_plan.h"

using namespace mrnnt;

namespace {

RNNTStatus check_pointers(const mrnnt_problem *p) {
    if (!p->acts) return fail(RNNT_STATUS_INVALID_VALUE, "acts is null");
    if (!p->T_dev || !p->S_dev) return fail(RNNT_STATUS_INVALID_VALUE, "device lengths are required");
    if (!p->labels) return fail(RNNT_STATUS_INVALID_VALUE, "labels is null");
    return RNNT_STATUS_SUCCESS;
}

// A launch that plans device-resident lengths itself (the chase, the fused log-softmax; walk_columns in
// mrnnt_device.h): the validation limits and the status report of the setup kernel, in the launch's view.
RNNTStatus plan_in_launch(const mrnnt_problem *p, const Plan &pl, int64_t scatter_above, DevProblem *d) {
    d->s_cap = pl.S_max;
    d->t_cap = pl.pad_S1 ? pl.pad_T : 0;
    d->s1_cap = pl.pad_S1;
    d->scatter_above = scatter_above;
    return status_device_ptr(p, &d->status_host);
}

// An asynchronous device-to-device copy into an output that may be NULL (then nothing to do).
// The row state of the tracked backward entry points: one byte per row of grads the call covers.
RNNTStatus check_row_state(const DevProblem &d, const unsigned char *row_state, int64_t row_state_len) {
    if (row_state && row_state_len < grads_rows(d))
        return fail(RNNT_STATUS_INVALID_VALUE, "row_state has " + std::to_string(row_state_len) + " bytes but the call covers " +
                                                   std::to_string(grads_rows(d)) + " rows of grads");
    return RNNT_STATUS_SUCCESS;
}

bool copy_out(void *dst, const void *src, size_t bytes, hipStream_t stream) {
    return !dst || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream) == hipSuccess;
}

// The tail of every dense gradient entry point, after its own checks: the row state, `before` (what the caller still
// launches ahead of the pass), the pass's column order, launch(d, grid) counted under K_GRAD ("<what> kernel" on
// failure), then the padding rows of the padded layout. grid 0: the persistent grid over the plan's columns.
template <class Launch, class Before>
RNNTStatus gradient_pass(const Plan &pl, DevProblem &d, unsigned char *row_state, int64_t row_state_len, void *grads,
                         int grid, const char *what, hipStream_t stream, Launch &&launch, Before &&before) {
    RNNTStatus st = check_row_state(d, row_state, row_state_len);
    if (st != RNNT_STATUS_SUCCESS) return st;
    d.row_state = row_state;
    if ((st = before()) != RNNT_STATUS_SUCCESS) return st;
    d.col_mul = column_order(pl, 2);
    if (grid == 0) grid = streaming_grid(pl.cols, tuning().grad_grid_per_cu);
    hipError_t e = timed(K_GRAD, stream, [&] { return launch(d, grid); });
    if (e != hipSuccess) return fail_hip(e, what);
    if (pl.pad_S1 != 0) {
        e = launch_pad_zero(d, pl.elem, grads, stream);
        if (e != hipSuccess) return fail_hip(e, "padding-rows zero kernel");
    }
    return RNNT_STATUS_SUCCESS;
}

template <class Launch>
RNNTStatus gradient_pass(const Plan &pl, DevProblem &d, unsigned char *row_state, int64_t row_state_len, void *grads,
                         int grid, const char *what, hipStream_t stream, Launch &&launch) {
    return gradient_pass(pl, d, row_state, row_state_len, grads, grid, what, stream, launch,
                         [] { return RNNT_STATUS_SUCCESS; });
}

// mrnnt_forward / mrnnt_hat_forward. hat: the factorised-blank log-softmax (DevProblem::hat) on every route but the
// chase launch, which has no factorised body: such a call takes the separate log-softmax + recursion.
RNNTStatus forward_impl(const mrnnt_problem *p, void *ws, size_t ws_bytes, float *costs_dev, int with_beta,
                        hipStream_t stream, bool hat) {
    Plan pl;
    RNNTStatus st = make_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_pointers(p)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_workspace(ws, ws_bytes, pl.total)) != RNNT_STATUS_SUCCESS) return st;
    DevProblem d = make_dev(p, pl, ws);
    d.hat = hat ? 1 : 0;
    hipError_t e = hipSuccess;
    // device-resident lengths of a small batch without an alignment: planned inside the log-softmax launch itself
    // (every wave holds the lengths in registers, walk_columns in mrnnt_device.h) -- no separate setup kernel, whose
    // ~4.7 us launch would be 5 % of a configs[1] step; otherwise one setup kernel before the passes
    const bool fused = pl.dyn && pl.B <= 64 && !pl.align && tuning().softmax_grid_per_cu <= 0 && tuning().dyn_fused;
    // the scattered order only matters where a workgroup walks several columns: the gradient's persistent grid
    // (the log-softmax's default is in order)
    const int64_t scatter_above = grad_scatter_above(pl);
    if (!fused) {
        LatticeOpts o;
        o.scatter_above = scatter_above;
        if ((st = prepare_lattice(p, pl, d, ws, o, stream)) != RNNT_STATUS_SUCCESS) return st;
    }
    // no alignment: the forward as one launch, the recursion chasing the log-softmax (mrnnt_chase.hip), where it has a
    // body for these rows and pays (chase_pays); with device lengths the launch also plans and validates them
    if (!hat && tuning().chase && chase_body(d, pl.elem) >= 0 && chase_pays(pl, with_beta) && (!pl.dyn || fused)) {
        ChaseArgs ca;
        ca.flags = carve<unsigned long long>(ws, pl.off_flags);
        // device lengths: the slots come from the lengths on the device; the grid from the plan's column bound
        // (min_cols; + B for the middle frames of odd T)
        const int64_t slot_bound = pl.dyn ? min_cols(pl) + pl.B : chase_slots(pl.B, pl.T_max, with_beta ? 1 : 0);
        ca.slots = pl.dyn ? 0 : slot_bound;
        ca.epoch = chase_epoch();
        ca.budget = (uint32_t)std::min<int64_t>((int64_t)std::max(0, tuning().chase_wait_us) * 100, UINT32_MAX / 2);
        ca.delay = kVariants ? (uint32_t)std::max(0, tuning().chase_delay_us) * 100u : 0u;
        ca.stage = kVariants ? tuning().chase_stage : 1;
        ca.probe = kVariants ? tuning().chase_probe : 0;
        ca.pair = kVariants ? tuning().chase_pair : 1;
        ca.early_free = kVariants ? tuning().chase_early_free : 1;
        ca.ring = kVariants ? tuning().chase_ring : 64;
        const int nrec = with_beta ? 2 * pl.B : pl.B;
        const int producers = (int)std::min<int64_t>(streaming_grid(slot_bound, tuning().chase_grid_per_cu),
                                                     ((int64_t)1 << 22) - nrec);
        DevProblem dc = d;
        if (pl.dyn && (st = plan_in_launch(p, pl, scatter_above, &dc)) != RNNT_STATUS_SUCCESS) return st;
        e = timed(K_CHASE, stream, [&] {
            return launch_chase(dc, ca, pl.elem, pl.S_max, with_beta ? 1 : 0, producers, costs_dev, stream);
        });
        if (e != hipSuccess) return fail_hip(e, "chase kernel");
        return RNNT_STATUS_SUCCESS;
    }
    if (fused) {
        // one workgroup per column at the lower bound of the column count (more columns are walked grid-stride)
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(min_cols(pl), 1 << 22));
        DevProblem ds = d;  // the log-softmax launch's view
        ds.dyn_fused = 1;
        ds.col_mul = 0;
        if ((st = plan_in_launch(p, pl, scatter_above, &ds)) != RNNT_STATUS_SUCCESS) return st;
        e = timed(K_SOFTMAX, stream, [&] { return launch_softmax(ds, pl.elem, grid, stream); });
        if (e != hipSuccess) return fail_hip(e, "log-softmax kernel");
    } else if ((st = softmax_pass(pl, d, stream)) != RNNT_STATUS_SUCCESS) {
        return st;
    }
    e = timed(K_DP, stream, [&] { return launch_dp(d, pl.S_max, with_beta ? 1 : 0, costs_dev, stream); });
    if (e != hipSuccess) return fail_hip(e, "alpha/beta kernel");
    return RNNT_STATUS_SUCCESS;
}

// mrnnt_backward_tracked / mrnnt_hat_backward_tracked. hat: the row policy HatRows (mrnnt_hat.hip).
RNNTStatus backward_impl(const mrnnt_problem *p, const void *ws, const float *grad_scale, void *grads,
                         unsigned char *row_state, int64_t row_state_len, hipStream_t stream, bool hat) {
    Plan pl;
    RNNTStatus st = make_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_pointers(p)) != RNNT_STATUS_SUCCESS) return st;
    if (!ws) return fail(RNNT_STATUS_INVALID_VALUE, "workspace is null");
    if (!grads) return fail(RNNT_STATUS_INVALID_VALUE, "grads is null");
    DevProblem d = make_dev(p, pl, ws);
    // grad_variant 3 sweeps rows (packed layout only), the others walk lattice columns (the factorised gradient always)
    const int grid = (!hat && tuning().grad_variant == 3 && pl.pad_S1 == 0)
                         ? streaming_grid(pl.N, std::max(1, tuning().grad_grid_per_cu))
                         : 0;
    return gradient_pass(pl, d, row_state, row_state_len, grads, grid, "gradient kernel", stream,
                         [&](const DevProblem &dv, int g) {
                             return hat ? launch_hat_grad(dv, pl.elem, grad_scale, grads, g, stream)
                                        : launch_grad(dv, pl.elem, grad_scale, grads, g, stream);
                         });
}

// mrnnt_align / mrnnt_hat_align
RNNTStatus align_impl(const mrnnt_problem *p, void *ws, size_t ws_bytes, int *alignment_out_dev, int64_t out_stride,
                      float *costs_dev, hipStream_t stream, bool hat) {
    Plan pl;
    RNNTStatus st = make_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_pointers(p)) != RNNT_STATUS_SUCCESS) return st;
    if (!alignment_out_dev) return fail(RNNT_STATUS_INVALID_VALUE, "alignment_out is null");
    if ((st = check_row_stride("alignment_out", out_stride, "input", pl.T_max, pl.dyn, 1)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_workspace(ws, ws_bytes, pl.total)) != RNNT_STATUS_SUCCESS) return st;
    DevProblem d = make_dev(p, pl, ws);
    d.hat = hat ? 1 : 0;
    // the separate-kernel route of mrnnt_forward: setup, alignment band, log-softmax, then the Viterbi launch in the
    // recursion's place (no chase, no planning inside the log-softmax launch)
    LatticeOpts o;
    o.t_cap = out_stride;  // T_b <= out_stride joins the device validation
    if ((st = prepare_lattice(p, pl, d, ws, o, stream)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = softmax_pass(pl, d, stream)) != RNNT_STATUS_SUCCESS) return st;
    // p->alignment may be alignment_out_dev itself: the band kernels above have consumed it (stream order) and the
    // Viterbi launch reads only the band arrays
    const hipError_t e =
        timed(K_DP, stream, [&] { return launch_viterbi(d, pl.S_max, alignment_out_dev, out_stride, costs_dev, stream); });
    if (e != hipSuccess) return fail_hip(e, "viterbi kernel");
    return RNNT_STATUS_SUCCESS;
}

}  // namespace

extern "C" {

// mrnnt_version, mrnnt_last_error, mrnnt_lattice_bytes / mrnnt_lattice_host: mrnnt_entry.cpp (host-only)

RNNTStatus mrnnt_workspace_size(const mrnnt_problem *p, size_t *bytes) {
    return plan_total<Plan>(bytes, [&](Plan *pl) { return make_plan(p, pl); });
}

RNNTStatus mrnnt_forward(const mrnnt_problem *p, void *ws, size_t ws_bytes, float *costs_dev, int with_beta,
                         hipStream_t stream) {
    return forward_impl(p, ws, ws_bytes, costs_dev, with_beta, stream, false);
}

RNNTStatus mrnnt_hat_forward(const mrnnt_problem *p, void *ws, size_t ws_bytes, float *costs_dev, int with_beta,
                             hipStream_t stream) {
    return forward_impl(p, ws, ws_bytes, costs_dev, with_beta, stream, true);
}

RNNTStatus mrnnt_backward(const mrnnt_problem *p, const void *ws, const float *grad_scale, void *grads,
                          hipStream_t stream) {
    return mrnnt_backward_tracked(p, ws, grad_scale, grads, nullptr, 0, stream);
}

RNNTStatus mrnnt_backward_tracked(const mrnnt_problem *p, const void *ws, const float *grad_scale, void *grads,
                                  unsigned char *row_state, int64_t row_state_len, hipStream_t stream) {
    return backward_impl(p, ws, grad_scale, grads, row_state, row_state_len, stream, false);
}

RNNTStatus mrnnt_hat_backward(const mrnnt_problem *p, const void *ws, const float *grad_scale, void *grads,
                              hipStream_t stream) {
    return backward_impl(p, ws, grad_scale, grads, nullptr, 0, stream, true);
}

RNNTStatus mrnnt_hat_backward_tracked(const mrnnt_problem *p, const void *ws, const float *grad_scale, void *grads,
                                      unsigned char *row_state, int64_t row_state_len, hipStream_t stream) {
    return backward_impl(p, ws, grad_scale, grads, row_state, row_state_len, stream, true);
}

RNNTStatus mrnnt_cost_and_grad(const mrnnt_problem *p, void *ws, size_t ws_bytes, float *costs_dev, void *grads,
                               const float *grad_scale, hipStream_t stream) {
    RNNTStatus st = mrnnt_forward(p, ws, ws_bytes, costs_dev, grads != nullptr, stream);
    if (st != RNNT_STATUS_SUCCESS || grads == nullptr) return st;
    return mrnnt_backward(p, ws, grad_scale, grads, stream);
}

RNNTStatus mrnnt_align(const mrnnt_problem *p, void *ws, size_t ws_bytes, int *alignment_out_dev, int64_t out_stride,
                       float *costs_dev, hipStream_t stream) {
    return align_impl(p, ws, ws_bytes, alignment_out_dev, out_stride, costs_dev, stream, false);
}

RNNTStatus mrnnt_hat_align(const mrnnt_problem *p, void *ws, size_t ws_bytes, int *alignment_out_dev,
                           int64_t out_stride, float *costs_dev, hipStream_t stream) {
    return align_impl(p, ws, ws_bytes, alignment_out_dev, out_stride, costs_dev, stream, true);
}

RNNTStatus mrnnt_posteriors(const mrnnt_problem *p, const void *ws, float *blank_post_dev, float *label_post_dev,
                            float *emit_dev, int64_t emit_stride, float *label_time_dev, int64_t time_stride,
                            hipStream_t stream) {
    Plan pl;
    RNNTStatus st = make_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    // with device lengths the kernels bound every write by the strides instead (and raise the status word)
    if (emit_dev && (st = check_row_stride("emit", emit_stride, "input", pl.T_max, pl.dyn, 0)) != RNNT_STATUS_SUCCESS)
        return st;
    if (label_time_dev &&
        (st = check_row_stride("label_time", time_stride, "label", pl.S_max, pl.dyn, 0)) != RNNT_STATUS_SUCCESS)
        return st;
    if (!ws) return fail(RNNT_STATUS_INVALID_VALUE, "workspace is null");
    if (!p->T_dev || !p->S_dev) return fail(RNNT_STATUS_INVALID_VALUE, "device lengths are required");
    DevProblem d = make_dev(p, pl, ws);  // acts and labels are never read
    if (pl.dyn && (st = status_device_ptr(p, &d.status_host)) != RNNT_STATUS_SUCCESS) return st;
    return posterior_readout(pl, d, {blank_post_dev, label_post_dev, emit_dev, emit_stride, label_time_dev, time_stride},
                             stream);
}

RNNTStatus mrnnt_sample(const mrnnt_problem *p, const void *ws, int num_samples, uint64_t seed, int64_t first_sample,
                        int *alignments_dev, int64_t out_stride, float *path_costs_dev, hipStream_t stream) {
    Plan pl;
    const RNNTStatus st = make_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return sample_readout(p, pl, ws, num_samples, seed, first_sample, alignments_dev, out_stride, path_costs_dev,
                          stream);
}

}  // extern "C"

namespace {

// mrnnt_path_*: the loss's plan with band arrays (the hull of the paths), then the per-path words.
struct PathPlan {
    Plan pl;
    size_t off_valid = 0, off_carry = 0, total = 0;
};

// The plan and the host checks of the path entry points, all before any device call.
RNNTStatus make_path_plan(const mrnnt_problem *p, int num_paths, PathPlan *pp) {
    const Plan &pl = pp->pl;
    const RNNTStatus st = plan_paths(p && p->alignment, num_paths, pl, [&] { return make_plan(p, &pp->pl, true); });
    if (st != RNNT_STATUS_SUCCESS) return st;
    Carver c{pl.total};
    pp->off_valid = c.take(sizeof(int) * (size_t)pl.B * num_paths);
    pp->off_carry = c.take(sizeof(int) * (size_t)path_carry_slots(pl.cols, pl.B) * num_paths);
    pp->total = c.at;
    return RNNT_STATUS_SUCCESS;
}

PathArgs path_args(const PathPlan &pp, void *ws, const int *alignments_dev, int num_paths, int64_t path_stride) {
    return mrnnt::path_args(ws, pp.off_valid, pp.off_carry, pp.pl.off_min, pp.pl.off_max, alignments_dev, num_paths,
                            path_stride);
}

// mrnnt_path_forward / mrnnt_hat_path_forward. hat: the factorised-blank log-softmax (DevProblem::hat) over the hull;
// the walk, hull and score kernels read lp and the band arrays only and serve both.
RNNTStatus path_forward_impl(const mrnnt_problem *p, void *ws, size_t ws_bytes, const int *alignments_dev,
                             int num_paths, int64_t path_stride, float *path_costs_dev, hipStream_t stream, bool hat) {
    PathPlan pp;
    RNNTStatus st = make_path_plan(p, num_paths, &pp);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const Plan &pl = pp.pl;
    if ((st = check_paths(pl, alignments_dev, path_stride)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_pointers(p)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_workspace(ws, ws_bytes, pp.total)) != RNNT_STATUS_SUCCESS) return st;
    DevProblem d = make_dev(p, pl, ws);  // d.min_s / d.max_s: the hull
    d.hat = hat ? 1 : 0;
    LatticeOpts o;
    o.t_cap = path_stride;
    o.scatter_above = grad_scatter_above(pl);  // the gradient's column order, as mrnnt_forward
    if ((st = prepare_lattice(p, pl, d, ws, o, stream)) != RNNT_STATUS_SUCCESS) return st;
    PathArgs a = path_args(pp, ws, alignments_dev, num_paths, path_stride);
    a.costs = path_costs_dev;
    hipError_t e = timed(K_DP, stream, [&] { return launch_path_walk(d, a, pl.T_max, stream); });
    if (e != hipSuccess) return fail_hip(e, "path walk kernels");
    // the log-softmax over the hull rows: the launch of mrnnt_align, its alignment window the hull
    if ((st = softmax_pass(pl, d, stream)) != RNNT_STATUS_SUCCESS) return st;
    if (path_costs_dev) {
        e = timed(K_DP, stream, [&] { return launch_path_score(d, a, stream); });
        if (e != hipSuccess) return fail_hip(e, "path score kernel");
    }
    return RNNT_STATUS_SUCCESS;
}

// mrnnt_path_backward_tracked / mrnnt_hat_path_backward_tracked. hat: the row policy HatPathRows (mrnnt_path.hip).
RNNTStatus path_backward_impl(const mrnnt_problem *p, void *ws, size_t ws_bytes, const int *alignments_dev,
                              int num_paths, int64_t path_stride, const float *weights_dev, void *grads,
                              unsigned char *row_state, int64_t row_state_len, hipStream_t stream, bool hat) {
    PathPlan pp;
    RNNTStatus st = make_path_plan(p, num_paths, &pp);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const Plan &pl = pp.pl;
    if ((st = check_paths(pl, alignments_dev, path_stride)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_pointers(p)) != RNNT_STATUS_SUCCESS) return st;
    if (!grads) return fail(RNNT_STATUS_INVALID_VALUE, "grads is null");
    if ((st = check_workspace(ws, ws_bytes, pp.total)) != RNNT_STATUS_SUCCESS) return st;
    DevProblem d = make_dev(p, pl, ws);
    PathArgs a = path_args(pp, ws, alignments_dev, num_paths, path_stride);
    a.w = weights_dev;
    return gradient_pass(
        pl, d, row_state, row_state_len, grads, 0, "path gradient kernel", stream,
        [&](const DevProblem &dv, int g) {
            return hat ? launch_hat_path_grad(dv, pl.elem, grads, g, stream)
                       : launch_path_grad(dv, pl.elem, grads, g, stream);
        },
        [&] {
            const hipError_t e = timed(K_DP, stream, [&] { return launch_path_coef(d, a, pl.T_max, stream); });
            return e != hipSuccess ? fail_hip(e, "path coefficient kernel") : RNNT_STATUS_SUCCESS;
        });
}

}  // namespace

extern "C" {

RNNTStatus mrnnt_path_workspace_size(const mrnnt_problem *p, int num_paths, size_t *bytes) {
    return plan_total<PathPlan>(bytes, [&](PathPlan *pp) { return make_path_plan(p, num_paths, pp); });
}

RNNTStatus mrnnt_path_forward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const int *alignments_dev,
                              int num_paths, int64_t path_stride, float *path_costs_dev, hipStream_t stream) {
    return path_forward_impl(p, ws, ws_bytes, alignments_dev, num_paths, path_stride, path_costs_dev, stream, false);
}

RNNTStatus mrnnt_hat_path_forward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const int *alignments_dev,
                                  int num_paths, int64_t path_stride, float *path_costs_dev, hipStream_t stream) {
    return path_forward_impl(p, ws, ws_bytes, alignments_dev, num_paths, path_stride, path_costs_dev, stream, true);
}

RNNTStatus mrnnt_path_backward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const int *alignments_dev,
                               int num_paths, int64_t path_stride, const float *weights_dev, void *grads,
                               hipStream_t stream) {
    return mrnnt_path_backward_tracked(p, ws, ws_bytes, alignments_dev, num_paths, path_stride, weights_dev, grads,
                                       nullptr, 0, stream);
}

RNNTStatus mrnnt_path_backward_tracked(const mrnnt_problem *p, void *ws, size_t ws_bytes, const int *alignments_dev,
                                       int num_paths, int64_t path_stride, const float *weights_dev, void *grads,
                                       unsigned char *row_state, int64_t row_state_len, hipStream_t stream) {
    return path_backward_impl(p, ws, ws_bytes, alignments_dev, num_paths, path_stride, weights_dev, grads, row_state,
                              row_state_len, stream, false);
}

RNNTStatus mrnnt_hat_path_backward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const int *alignments_dev,
                                   int num_paths, int64_t path_stride, const float *weights_dev, void *grads,
                                   hipStream_t stream) {
    return path_backward_impl(p, ws, ws_bytes, alignments_dev, num_paths, path_stride, weights_dev, grads, nullptr, 0,
                              stream, true);
}

RNNTStatus mrnnt_hat_path_backward_tracked(const mrnnt_problem *p, void *ws, size_t ws_bytes,
                                           const int *alignments_dev, int num_paths, int64_t path_stride,
                                           const float *weights_dev, void *grads, unsigned char *row_state,
                                           int64_t row_state_len, hipStream_t stream) {
    return path_backward_impl(p, ws, ws_bytes, alignments_dev, num_paths, path_stride, weights_dev, grads, row_state,
                              row_state_len, stream, true);
}

}  // extern "C"

namespace {

// mrnnt_expect_*: the loss's plan (a restricting alignment included), then the expectation state A / Bk / R.
struct ExpectPlan {
    Plan pl;
    ExpectState state;
    size_t total = 0;
};

RNNTStatus make_expect_plan(const mrnnt_problem *p, ExpectPlan *ep) {
    const RNNTStatus st = make_plan(p, &ep->pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    Carver c{ep->pl.total};
    ep->state.carve_from(&c, ep->pl);
    ep->total = c.at;
    return RNNT_STATUS_SUCCESS;
}

// mrnnt_expect_forward / mrnnt_hat_expect_forward. hat: the forward is mrnnt_hat_forward's (never the chase launch);
// the expectation recursion reads alpha / beta / lp and the costs only and serves both.
RNNTStatus expect_forward_impl(const mrnnt_problem *p, void *ws, size_t ws_bytes, const float *blank_cost_dev,
                               const float *label_cost_dev, float *expected_dev, float *costs_dev, int with_grad,
                               hipStream_t stream, bool hat) {
    ExpectPlan ep;
    RNNTStatus st = make_expect_plan(p, &ep);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_pointers(p)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_workspace(ws, ws_bytes, ep.total)) != RNNT_STATUS_SUCCESS) return st;
    // the loss's forward on the head of the workspace (its own plan: the same offsets), beta only for a gradient
    if ((st = forward_impl(p, ws, ws_bytes, costs_dev, with_grad ? 1 : 0, stream, hat)) != RNNT_STATUS_SUCCESS) return st;
    DevProblem d = make_dev(p, ep.pl, ws);
    ep.state.bind(&d, ws, blank_cost_dev, label_cost_dev);
    const hipError_t e =
        timed(K_DP, stream, [&] { return launch_expect(d, ep.pl.S_max, with_grad ? 1 : 0, expected_dev, stream); });
    if (e != hipSuccess) return fail_hip(e, "expectation recursion kernel");
    return RNNT_STATUS_SUCCESS;
}

// mrnnt_expect_backward_tracked / mrnnt_hat_expect_backward_tracked. hat: the row policy HatExpectRows (mrnnt_expect.hip).
RNNTStatus expect_backward_impl(const mrnnt_problem *p, void *ws, size_t ws_bytes, const float *blank_cost_dev,
                                const float *label_cost_dev, const float *grad_expected_dev,
                                const float *grad_costs_dev, void *grads, unsigned char *row_state,
                                int64_t row_state_len, hipStream_t stream, bool hat) {
    ExpectPlan ep;
    RNNTStatus st = make_expect_plan(p, &ep);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const Plan &pl = ep.pl;
    if ((st = check_pointers(p)) != RNNT_STATUS_SUCCESS) return st;
    if (!grads) return fail(RNNT_STATUS_INVALID_VALUE, "grads is null");
    if ((st = check_workspace(ws, ws_bytes, ep.total)) != RNNT_STATUS_SUCCESS) return st;
    DevProblem d = make_dev(p, pl, ws);
    ep.state.bind(&d, ws, blank_cost_dev, label_cost_dev);
    d.ex_ge = grad_expected_dev;
    d.ex_gc = grad_costs_dev;
    return gradient_pass(pl, d, row_state, row_state_len, grads, 0, "expected-cost gradient kernel", stream,
                         [&](const DevProblem &dv, int g) {
                             return hat ? launch_hat_expect_grad(dv, pl.elem, grads, g, stream)
                                        : launch_expect_grad(dv, pl.elem, grads, g, stream);
                         });
}

}  // namespace

extern "C" {

RNNTStatus mrnnt_expect_workspace_size(const mrnnt_problem *p, size_t *bytes) {
    return plan_total<ExpectPlan>(bytes, [&](ExpectPlan *ep) { return make_expect_plan(p, ep); });
}

RNNTStatus mrnnt_expect_forward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const float *blank_cost_dev,
                                const float *label_cost_dev, float *expected_dev, float *costs_dev, int with_grad,
                                hipStream_t stream) {
    return expect_forward_impl(p, ws, ws_bytes, blank_cost_dev, label_cost_dev, expected_dev, costs_dev, with_grad,
                               stream, false);
}

RNNTStatus mrnnt_hat_expect_forward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const float *blank_cost_dev,
                                    const float *label_cost_dev, float *expected_dev, float *costs_dev, int with_grad,
                                    hipStream_t stream) {
    return expect_forward_impl(p, ws, ws_bytes, blank_cost_dev, label_cost_dev, expected_dev, costs_dev, with_grad,
                               stream, true);
}

RNNTStatus mrnnt_expect_backward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const float *blank_cost_dev,
                                 const float *label_cost_dev, const float *grad_expected_dev,
                                 const float *grad_costs_dev, void *grads, hipStream_t stream) {
    return mrnnt_expect_backward_tracked(p, ws, ws_bytes, blank_cost_dev, label_cost_dev, grad_expected_dev,
                                         grad_costs_dev, grads, nullptr, 0, stream);
}

RNNTStatus mrnnt_expect_backward_tracked(const mrnnt_problem *p, void *ws, size_t ws_bytes, const float *blank_cost_dev,
                                         const float *label_cost_dev, const float *grad_expected_dev,
                                         const float *grad_costs_dev, void *grads, unsigned char *row_state,
                                         int64_t row_state_len, hipStream_t stream) {
    return expect_backward_impl(p, ws, ws_bytes, blank_cost_dev, label_cost_dev, grad_expected_dev, grad_costs_dev,
                                grads, row_state, row_state_len, stream, false);
}

RNNTStatus mrnnt_hat_expect_backward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const float *blank_cost_dev,
                                     const float *label_cost_dev, const float *grad_expected_dev,
                                     const float *grad_costs_dev, void *grads, hipStream_t stream) {
    return expect_backward_impl(p, ws, ws_bytes, blank_cost_dev, label_cost_dev, grad_expected_dev, grad_costs_dev,
                                grads, nullptr, 0, stream, true);
}

RNNTStatus mrnnt_hat_expect_backward_tracked(const mrnnt_problem *p, void *ws, size_t ws_bytes,
                                             const float *blank_cost_dev, const float *label_cost_dev,
                                             const float *grad_expected_dev, const float *grad_costs_dev, void *grads,
                                             unsigned char *row_state, int64_t row_state_len, hipStream_t stream) {
    return expect_backward_impl(p, ws, ws_bytes, blank_cost_dev, label_cost_dev, grad_expected_dev, grad_costs_dev,
                                grads, row_state, row_state_len, stream, true);
}

RNNTStatus mrnnt_read_loglik(const mrnnt_problem *p, const void *ws, double *ll_fwd_dev, double *ll_bwd_dev,
                             hipStream_t stream) {
    Plan pl;
    RNNTStatus st = make_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const char *w = static_cast<const char *>(ws);
    if (!copy_out(ll_fwd_dev, w + pl.off_ll, sizeof(double) * pl.B, stream))
        return fail(RNNT_STATUS_MEMOPS_FAILED, "copy ll_fwd");
    if (!copy_out(ll_bwd_dev, w + pl.off_llb, sizeof(double) * pl.B, stream))
        return fail(RNNT_STATUS_MEMOPS_FAILED, "copy ll_bwd");
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_read_state(const mrnnt_problem *p, const void *ws, float *den_dev, double *alpha_dev,
                            double *beta_dev, hipStream_t stream) {
    Plan pl;
    RNNTStatus st = make_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (!ws) return fail(RNNT_STATUS_INVALID_VALUE, "workspace is null");
    const DevProblem d = make_dev(p, pl, ws);
    if (!copy_out(den_dev, d.den, sizeof(float) * pl.N, stream)) return fail(RNNT_STATUS_MEMOPS_FAILED, "copy den");
    if (!copy_out(alpha_dev, d.alpha, sizeof(double) * pl.N, stream))
        return fail(RNNT_STATUS_MEMOPS_FAILED, "copy alpha");
    if (!copy_out(beta_dev, d.beta, sizeof(double) * pl.N, stream)) return fail(RNNT_STATUS_MEMOPS_FAILED, "copy beta");
    if ((alpha_dev || beta_dev) && launch_mask_state(d, alpha_dev, beta_dev, stream) != hipSuccess)
        return fail(RNNT_STATUS_EXECUTION_FAILED, "mask state");
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_read_denoms(const mrnnt_problem *p, const void *ws, float *den_dev, hipStream_t stream) {
    Plan pl;
    RNNTStatus st = make_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_pointers(p)) != RNNT_STATUS_SUCCESS) return st;
    if (!ws || !den_dev) return fail(RNNT_STATUS_INVALID_VALUE, "workspace / den is null");
    const hipError_t e = launch_den_all(make_dev(p, pl, ws), pl.elem, den_dev, stream);
    if (e != hipSuccess) return fail_hip(e, "denominator read-out kernel");
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_read_band(const mrnnt_problem *p, void *ws, int *min_dev, int *max_dev, int64_t ld,
                           hipStream_t stream) {
    Plan pl;
    RNNTStatus st = make_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (!ws) return fail(RNNT_STATUS_INVALID_VALUE, "workspace is null");
    if (!p->T_dev || !p->S_dev) return fail(RNNT_STATUS_INVALID_VALUE, "device lengths are required");
    if (ld < 1 || (!pl.dyn && ld < pl.T_max))
        return fail(RNNT_STATUS_INVALID_VALUE, "band row stride " + std::to_string(ld) + " < max input length");
    DevProblem d = make_dev(p, pl, ws);
    // offsets + validation exactly as mrnnt_forward builds them, but an inspection call: it leaves the lp array (the
    // state of an earlier forward) and the status word alone, and stays out of the profile
    LatticeOpts o;
    o.zero_lp_pads = o.report_status = o.timed = false;
    if ((st = prepare_lattice(p, pl, d, ws, o, stream)) != RNNT_STATUS_SUCCESS) return st;
    const hipError_t e = launch_band_read(d, min_dev, max_dev, ld, stream);
    if (e != hipSuccess) return fail_hip(e, "band read-out kernel");
    return RNNT_STATUS_SUCCESS;
}

int *mrnnt_status_word(void) { return process_status_word(); }

RNNTStatus mrnnt_grad_live_rows(const mrnnt_problem *p, const void *ws, unsigned long long *count_dev,
                                hipStream_t stream) {
    Plan pl;
    RNNTStatus st = make_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_pointers(p)) != RNNT_STATUS_SUCCESS) return st;
    if (!ws || !count_dev) return fail(RNNT_STATUS_INVALID_VALUE, "workspace / count is null");
    const hipError_t e = launch_count_live(make_dev(p, pl, ws), count_dev, stream);
    if (e != hipSuccess) return fail_hip(e, "live-row count kernel");
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_fill_zero(void *dst, size_t bytes, hipStream_t stream) {
    if (bytes == 0) return RNNT_STATUS_SUCCESS;
    if (!dst || (reinterpret_cast<uintptr_t>(dst) & 15) || (bytes & 15))
        return fail(RNNT_STATUS_INVALID_VALUE, "fill_zero: null or not 16-byte aligned pointer / size");
    const hipError_t e = launch_fill_zero(dst, bytes, streaming_grid((int64_t)1 << 40, 32), stream);
    if (e != hipSuccess) return fail_hip(e, "zero fill kernel");
    return RNNT_STATUS_SUCCESS;
}

#ifdef MRNNT_DEVTOOLS
// development build: columns chase recursion waves computed themselves since the last reset (mrnnt_chase.hip)
__attribute__((visibility("default"))) unsigned long long mrnnt_chase_helped(int reset) { return chase_helped(reset != 0); }
__attribute__((visibility("default"))) int mrnnt_chase_trace(unsigned long long *out, int n) { return chase_trace(out, n); }
__attribute__((visibility("default"))) int mrnnt_chase_walk_trace(unsigned long long *out, int n) {
    return chase_walk_trace(out, n);
}
__attribute__((visibility("default"))) int mrnnt_joint_trace(unsigned long long *out, int n) { return joint_trace(out, n); }
__attribute__((visibility("default"))) int mrnnt_joint_reduce_trace(unsigned long long *out, int n) {
    return joint_reduce_trace(out, n);
}

// launch knobs: exported by the development build only (libmonotonic_rnnt_amd_dev.so, `make dev`)
__attribute__((visibility("default"))) int mrnnt_tune(const char *key, int value) {
    if (!key) return -1;
    Tuning &t = tuning();
    if (!std::strcmp(key, "grid_per_cu")) {  // both streaming kernels
        const int prev = t.grad_grid_per_cu;
        if (value >= 0) t.softmax_grid_per_cu = t.grad_grid_per_cu = value;
        return prev;
    }
#define KNOB(name) {#name, &Tuning::name}
    static const struct {
        const char *key;
        int Tuning::*slot;
    } knobs[] = {KNOB(softmax_variant), KNOB(grad_variant), KNOB(col_scatter), KNOB(col_xcd), KNOB(dp_halo),
                 KNOB(dp_lean), KNOB(joint_reduce_sparse), KNOB(joint_dpre_nw), KNOB(joint_dpre_abl),
                 KNOB(joint_reduce_hact), KNOB(joint_probe), KNOB(joint_opt), KNOB(joint_trace),
                 KNOB(joint_reduce_pad), KNOB(softmax_grid_per_cu), KNOB(grad_grid_per_cu), KNOB(nt_store),
                 KNOB(dyn_fused), KNOB(chase), KNOB(chase_wait_us), KNOB(chase_stage), KNOB(chase_delay_us),
                 KNOB(chase_probe), KNOB(chase_pair), KNOB(chase_early_free), KNOB(chase_ring),
                 KNOB(chase_grid_per_cu), KNOB(nt_load), KNOB(occ_skip), KNOB(joint_bwd_mfma)};
#undef KNOB
    for (const auto &k : knobs) {
        if (std::strcmp(key, k.key)) continue;
        const int prev = t.*k.slot;
        if (value >= 0) t.*k.slot = value;
        return prev;
    }
    return -1;
}
#endif  // MRNNT_DEVTOOLS

}  // extern "C"
