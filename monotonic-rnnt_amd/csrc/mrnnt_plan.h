// mrnnt_plan.h -- what the host translation units of the GPU path share (mrnnt_capi.cpp: the flat loss ABI,
// mrnnt_joint_capi.cpp: the fused-joint ABI, mrnnt_manager.cpp: the reference-shaped C++ surface): validation and the
// workspace plan, the device-problem builder, the lattice preparation, the chase decision, launch grids, the status
// word and the per-launch profile. Defined in mrnnt_plan.cpp, which holds the one instance of every piece of
// process-wide state. Host only (the kernels include mrnnt_internal.h alone); hidden visibility; not part of the ABI.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#pragma GCC visibility push(default)
#include "mrnnt.h"
#pragma GCC visibility pop
#include "mrnnt_internal.h"

namespace mrnnt {

// this thread's mrnnt_last_error() (the error state lives in mrnnt_entry.cpp)
RNNTStatus fail(RNNTStatus st, const std::string &msg);
RNNTStatus fail_hip(hipError_t e, const char *where);

size_t align_up(size_t x);  // to the workspace's 256-byte granule

// Carves a workspace: take(bytes) is the offset of the next array (each on the granule), `at` ends as the total.
struct Carver {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t off = at;
        at = align_up(at + bytes);
        return off;
    }
};

// A *_workspace_size entry point: the total of the plan that `make` fills.
template <class PlanT, class F>
RNNTStatus plan_total(size_t *bytes, F &&make) {
    if (!bytes) return fail(RNNT_STATUS_INVALID_VALUE, "null size pointer");
    PlanT pl;
    const RNNTStatus st = make(&pl);
    if (st == RNNT_STATUS_SUCCESS) *bytes = pl.total;
    return st;
}

// Rows of one utterance inside the monotonic band: sum_t min(t, S) - max(0, t - (T - S)) + 1.
int64_t inband_rows(int T, int S);

// Launch plan of one problem. With host lengths every size is exact. With device-resident lengths
// (lengths_on_device) the host plans from bounds it knows without a read-back: N = the rows of acts (packed: exact,
// checked on the device; padded: B*pad_T*pad_S1), cols <= N (packed; every column holds >= 1 row) or B*pad_T
// (padded), S_max <= label_stride; the setup kernel publishes the real values (DynWords) for the kernels.
struct Plan {
    int B = 0, V = 0, S_max = 0, T_max = 0;
    int64_t N = 0, cols = 0;
    int elem = ELEM_F32;
    int64_t pad_T = 0, pad_S1 = 0;
    bool align = false;
    bool dyn = false;
    size_t off_flags = 0, flags_bytes = 0;  // the chase launch's ready flags (8 bytes per column), where it can run
    size_t off_row, off_col, off_colb, off_mtmp, off_min, off_max, off_den, off_lp, off_alpha, off_beta, off_ll,
        off_llb, off_dyn, total;
};

// band: the plan holds the band arrays (min_s / max_s) although the problem has no alignment (mrnnt_path_*: the
// hull of the given paths goes there)
RNNTStatus make_plan(const mrnnt_problem *p, Plan *pl, bool band = false);
DevProblem make_dev(const mrnnt_problem *p, const Plan &pl, const void *ws);

// The array at byte offset `off` of a workspace.
template <class T>
T *carve(void *ws, size_t off) {
    return reinterpret_cast<T *>(static_cast<char *>(ws) + off);
}

// "workspace too small" unless ws holds `need` bytes
RNNTStatus check_workspace(const void *ws, size_t ws_bytes, size_t need);

// Lower bound on the column count that the host knows with device lengths: rows / (label stride + 1), exact when
// every S_b equals the stride, or B * pad_T for the padded layout.
int64_t min_cols(const Plan &pl);

// The chase launch (mrnnt_chase.hip): whether it pays for this call (the plan holds its ready flags where its shape
// can take it at all), and a fresh tag per launch.
bool chase_pays(const Plan &pl, bool with_beta);
uint64_t chase_epoch();

// Column order of a streaming pass (DevProblem::col_mul): XCD-chunked (< 0), scattered (> 0: with device lengths a
// marker the kernels replace by the device's multiplier, resolve_dyn) or in order (0). bit: 1 log-softmax, 2 gradient.
int64_t column_order(const Plan &pl, int bit);

// per_cu workgroups of 4 waves per CU walking `cols` columns grid-stride, never more than the columns; per_cu == 0:
// one workgroup per column (hardware-scheduled)
int streaming_grid(int64_t cols, int per_cu);

// The gradient's DynSetupArgs::scatter_above for the plan: its persistent grid where it walks a scattered order.
int64_t grad_scatter_above(const Plan &pl);

// A caller's row stride against the longest length it has to hold: "<what> row stride N < max <of> length M". With
// device lengths only the lower limit `least` (0 or 1) is known on the host (the kernels bound the rest).
RNNTStatus check_row_stride(const char *what, int64_t stride, const char *of, int64_t need, bool dyn, int least);

// Device address of a caller's status word (host-mapped memory), nullptr for none.
RNNTStatus status_device_ptr(const mrnnt_problem *p, int **dev);
int *process_status_word();  // mrnnt_status_word(): one host-mapped word per process

// The lattice offsets and the alignment band of a call, in its workspace: exactly one of the device-lengths setup
// kernel, the host-lengths setup kernel (no caller lattice) or nothing (a caller lattice), then the band kernels when
// the plan has an alignment. What the entry points do differently is all here:
struct LatticeOpts {
    int64_t t_cap = 0;                   // one more bound on T_b for the device validation (0 = none)
    int64_t scatter_above = INT64_MAX;   // DynSetupArgs::scatter_above (INT64_MAX: no gradient pass follows)
    bool zero_lp_pads = true;            // device lengths: the setup kernel zeroes the pads of the lp array
    bool report_status = true;           // device lengths: a failed validation raises the caller's status word
    bool timed = true;                   // the launches count in the profile (K_SETUP, K_BAND)
};
RNNTStatus prepare_lattice(const mrnnt_problem *p, const Plan &pl, const DevProblem &d, void *ws,
                           const LatticeOpts &o, hipStream_t stream);

// The log-softmax pass over a lattice prepared by prepare_lattice (counted under K_SOFTMAX): one workgroup per column,
// or with device lengths a work-stealing grid (the column count is not known on the host).
RNNTStatus softmax_pass(const Plan &pl, const DevProblem &d, hipStream_t stream);

// mrnnt_posteriors / mrnnt_joint_posteriors after their checks: the read-out launch (counted under K_DP).
RNNTStatus posterior_readout(const Plan &pl, const DevProblem &d, const PosteriorArgs &a, hipStream_t stream);

// mrnnt_sample / mrnnt_joint_sample after their plans: the host checks (before any device call), then the sampler
// launch on the plan's lattice (counted under K_DP).
RNNTStatus sample_readout(const mrnnt_problem *p, const Plan &pl, const void *ws, int num_samples, uint64_t seed,
                          int64_t first_sample, int *alignments_dev, int64_t out_stride, float *path_costs_dev,
                          hipStream_t stream);

// mrnnt_path_* / mrnnt_joint_path_*: the host check of the caller's alignment rows (non-NULL, path_stride >= max T_b;
// with device lengths T_b <= path_stride joins the device validation), and the path launches' arguments over a
// workspace that holds the per-path words and the hull (band) arrays at the given offsets.
RNNTStatus check_paths(const Plan &pl, const int *alignments_dev, int64_t path_stride);
PathArgs path_args(void *ws, size_t off_valid, size_t off_carry, size_t off_min, size_t off_max,
                   const int *alignments_dev, int num_paths, int64_t path_stride);

// The preconditions of the path entry points around the plan `make` fills into pl, in their order: no restricting
// alignment, num_paths >= 1, the plan's own checks, then the batch limits of the path kernels.
template <class F>
RNNTStatus plan_paths(bool restricted, int num_paths, const Plan &pl, F &&make) {
    if (restricted)
        return fail(RNNT_STATUS_INVALID_VALUE, "path scores take no restricting alignment (p->alignment must be NULL: "
                                               "the band arrays hold the hull of the given paths)");
    if (num_paths < 1)
        return fail(RNNT_STATUS_INVALID_VALUE, "num_paths must be >= 1, got " + std::to_string(num_paths));
    const RNNTStatus st = make();
    if (st != RNNT_STATUS_SUCCESS) return st;
    if ((int64_t)pl.B * num_paths > 0x7fffffff || pl.B > 65535)
        return fail(RNNT_STATUS_INVALID_VALUE, "path scores take B <= 65535 and B * num_paths < 2^31");
    return RNNT_STATUS_SUCCESS;
}

// mrnnt_expect_* / mrnnt_joint_expect_*: the expectation state A / Bk (fp64 [N]) and R (fp64 [B]) carved after a
// plan's own arrays, and the device problem's view of it and of the caller's cost arrays.
struct ExpectState {
    size_t off_A = 0, off_Bk = 0, off_R = 0;
    void carve_from(Carver *c, const Plan &pl);
    void bind(DevProblem *d, void *ws, const float *blank_cost_dev, const float *label_cost_dev) const;
};

// A caller's grid [B, grid_T, grid_S1] holds every row of the lattice (not looked at unless `given`):
// "<noun> grid [..] smaller than [max T, max S + 1] = [..]"
RNNTStatus check_grid(const Plan &pl, bool given, const char *noun, int64_t grid_T, int64_t grid_S1);

// ---- profiling (mrnnt_profile_enable / mrnnt_profile_read) ------------------------------------------------------
struct ProfRec {
    int id;
    hipEvent_t a, b;
};
// false when the profile is off (or out of events); else r->a is recorded on s and profile_end records r->b
bool profile_begin(int id, hipStream_t s, ProfRec *r);
void profile_end(const ProfRec &r, hipStream_t s);

template <class F>
hipError_t timed(int id, hipStream_t s, F &&launch) {
    ProfRec r;
    if (!profile_begin(id, s, &r)) return launch();
    const hipError_t e = launch();
    profile_end(r, s);
    return e;
}

}  // namespace mrnnt
