// mrnnt_plan.cpp -- the shared host side of the GPU path (mrnnt_plan.h): validation and workspace plan, the
// device-problem builder, the lattice preparation, the chase decision, launch grids, and the process-wide state
// (status word, profile events, chase epoch counter), each with its one instance here.
#include "mrnnt_plan.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include <random>
#include <vector>

namespace mrnnt {

RNNTStatus fail(RNNTStatus st, const std::string &msg) { return set_error(st, msg); }

RNNTStatus fail_hip(hipError_t e, const char *where) {
    return fail(RNNT_STATUS_EXECUTION_FAILED, std::string(where) + ": " + hipGetErrorString(e));
}

constexpr size_t kAlign = 256;
size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

RNNTStatus check_workspace(const void *ws, size_t ws_bytes, size_t need) {
    if (ws && ws_bytes >= need) return RNNT_STATUS_SUCCESS;
    return fail(RNNT_STATUS_INVALID_VALUE, "workspace too small: need " + std::to_string(need) + " bytes");
}

// ---- device properties -------------------------------------------------------------------------

static int cu_count() {  // of the current device
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (cached[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev] = n;
    }
    return cached[dev];
}

int streaming_grid(int64_t cols, int per_cu) {
    // (the hardware-scheduled grid is capped at 2^22 workgroups: the dispatch size in work-items is 32-bit, and
    // every streaming kernel walks its columns grid-stride, so larger problems just take more than one turn)
    const int64_t g = per_cu <= 0 ? std::min<int64_t>(cols, 1 << 22) : (int64_t)cu_count() * per_cu;
    return (int)std::max<int64_t>(1, std::min<int64_t>(g, cols));
}

int64_t min_cols(const Plan &pl) { return pl.pad_S1 ? pl.cols : (pl.N + pl.S_max) / (pl.S_max + 1); }

// Mean frames per utterance: exact with host lengths; with device lengths the plan's lower bound on the column count
// over B (pad_T for the padded layout).
static double mean_frames(const Plan &pl) { return (double)(pl.dyn ? min_cols(pl) : pl.cols) / pl.B; }

// The chase launch (mrnnt_chase.hip) where its shape allows it and it pays:
// * f32 rows it has a body for, no alignment band, the halo recursion in one 4-wave workgroup (S + 1 <= 4 * 56), the
//   lp array one buffer descriptor (N * 16 bytes < 2^31), device lengths for B <= 64 (one utterance per lane);
// * its recursion workgroups spin while they wait, so together they should leave the chip to the producers: at most
//   one per CU (B or 2B <= CUs). (Progress does not rely on it -- a starved recursion wave computes its columns
//   itself -- but a launch that has to is slow.)
// * it saves the recursion's time (~T steps of ~0.1 us) at the price of a slightly slower log-softmax pass (+5-10 %,
//   the hand-off and the production order): taken when the recursion is at least a quarter of the pass's streaming
//   time (configs[1]: 20 vs 22 us; the headline: 0.16 vs 6.5 ms, not taken).
static bool chase_shape_ok(const Plan &pl) {
    if (pl.align || pl.elem != ELEM_F32 || chase_body_shape(pl.V) < 0) return false;
    if (pl.S_max + 1 > 4 * 56 || pl.N * (int64_t)sizeof(Lp) >= ((int64_t)1 << 31)) return false;
    if (pl.dyn && pl.B > 64) return false;
    // one recursion workgroup per utterance and direction: the cost-only forward needs B of them, the gradient call 2B
    // (chase_pays decides per call). The flags are sized here, so the workspace size depends on the CU count of the
    // device current when the plan is made (a problem of B > CUs utterances never takes the chase).
    if (pl.B > cu_count()) return false;
    const double pass_s = (double)pl.N * pl.V * 4.0 / 6.0e12, recursion_s = mean_frames(pl) * 1.0e-7;
    return recursion_s >= 0.25 * pass_s;
}

bool chase_pays(const Plan &pl, bool with_beta) {
    return pl.flags_bytes && (with_beta ? 2 * pl.B : pl.B) <= cu_count();
}

// A fresh 64-bit tag per chase launch (mrnnt_chase.hip): a bijective mix of a process-wide counter whose start is
// random per process, so no two calls of a process share one and a stale word matches with probability 2^-64.
uint64_t chase_epoch() {
    static std::atomic<uint64_t> ctr{((uint64_t)std::random_device{}() << 32) ^ (uint64_t)std::random_device{}() ^
                                     (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count()};
    uint64_t x = ctr.fetch_add(1, std::memory_order_relaxed) * 0x9E3779B97F4A7C15ull;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x ? x : 1;
}

static RNNTStatus plan_device_lengths(const mrnnt_problem *p, Plan &q) {
    if (!p->T_dev || !p->S_dev) return fail(RNNT_STATUS_INVALID_VALUE, "device lengths are required");
    if (p->lattice)
        return fail(RNNT_STATUS_INVALID_VALUE, "lattice must be NULL with lengths_on_device (built on the device)");
    if (p->num_rows < 0) return fail(RNNT_STATUS_INVALID_VALUE, "num_rows is required with lengths_on_device");
    if (p->label_stride < 0) return fail(RNNT_STATUS_INVALID_VALUE, "negative label row stride");
    if (p->pad_S1 != 0) {
        if (p->pad_S1 < 1 || p->pad_T < 1) return fail(RNNT_STATUS_INVALID_VALUE, "padded layout needs pad_T, pad_S1 >= 1");
        q.N = (int64_t)p->B * p->pad_T * p->pad_S1;
        q.cols = (int64_t)p->B * p->pad_T;
        q.T_max = (int)std::min<int64_t>(p->pad_T, 1 << 30);
        q.S_max = (int)std::min<int64_t>(p->label_stride, p->pad_S1 - 1);
    } else {
        q.N = p->num_rows;
        q.cols = q.N;
        q.T_max = (int)std::min<int64_t>(q.N, 1 << 30);
        q.S_max = (int)std::min<int64_t>(p->label_stride, 1 << 30);
    }
    if (q.S_max + 1 > kMaxLabelsPlusOne)
        return fail(RNNT_STATUS_INVALID_VALUE, "with device lengths the label row stride (" +
                                                   std::to_string(p->label_stride) + ") bounds S_b and must be <= " +
                                                   std::to_string(kMaxLabelsPlusOne - 1) +
                                                   ": pass labels no wider than the longest label sequence");
    if (p->num_rows != q.N)
        return fail(RNNT_STATUS_INVALID_VALUE, "acts has " + std::to_string(p->num_rows) + " rows but the padded layout needs " +
                                                   std::to_string(q.N));
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus make_plan(const mrnnt_problem *p, Plan *pl, bool band) {
    if (!p) return fail(RNNT_STATUS_INVALID_VALUE, "null problem");
    if (p->B <= 0) return fail(RNNT_STATUS_INVALID_VALUE, "B must be > 0");
    if (p->V <= 0) return fail(RNNT_STATUS_INVALID_VALUE, "V must be > 0");
    const bool dyn = p->lengths_on_device != 0;
    if (!dyn && (!p->T_host || !p->S_host)) return fail(RNNT_STATUS_INVALID_VALUE, "host lengths are required");
    if (p->blank < 0 || p->blank >= p->V) return fail(RNNT_STATUS_INVALID_VALUE, "blank label out of range [0, V)");
    Plan q;
    q.B = p->B;
    q.V = p->V;
    q.dyn = dyn;
    if (dyn) {
        const RNNTStatus st = plan_device_lengths(p, q);
        if (st != RNNT_STATUS_SUCCESS) return st;
    }
    for (int b = 0; !dyn && b < p->B; ++b) {
        const int T = p->T_host[b], S = p->S_host[b];
        // reference validation: cpu_workspace_manager.h:103-107 / gpu_workspace_manager.h:235-239
        if (T <= 0 || S < 0 || T < S)
            return fail(RNNT_STATUS_INVALID_VALUE, "invalid lengths at utterance " + std::to_string(b) + ": T=" +
                                                       std::to_string(T) + " S=" + std::to_string(S) +
                                                       " (need T > 0, S >= 0, T >= S)");
        q.N += (int64_t)T * (S + 1);
        q.cols += T;
        q.S_max = std::max(q.S_max, S);
        q.T_max = std::max(q.T_max, T);
    }
    if (q.S_max + 1 > kMaxLabelsPlusOne)
        return fail(RNNT_STATUS_INVALID_VALUE, "max label length " + std::to_string(q.S_max) + " exceeds " +
                                                   std::to_string(kMaxLabelsPlusOne - 1));
    // the kernels read labels[b * label_stride + s] for s < S_b and alignment[b * align_stride + t] for t < T_b
    // (with device lengths the setup kernel checks S_b <= label_stride and T_b <= align_stride)
    if (q.S_max > 0 && p->label_stride < q.S_max)
        return fail(RNNT_STATUS_INVALID_VALUE, "label row stride " + std::to_string(p->label_stride) +
                                                   " < max label length " + std::to_string(q.S_max));
    if (!dyn && p->alignment && p->align_stride < q.T_max)
        return fail(RNNT_STATUS_INVALID_VALUE, "alignment row stride " + std::to_string(p->align_stride) +
                                                   " < max input length " + std::to_string(q.T_max));
    if (dyn && p->alignment && p->align_stride < 1)
        return fail(RNNT_STATUS_INVALID_VALUE, "alignment row stride must be >= 1");
    if (p->acts_dtype != ELEM_F32 && p->acts_dtype != ELEM_BF16 && p->acts_dtype != ELEM_F16)
        return fail(RNNT_STATUS_INVALID_VALUE, "unknown acts_dtype " + std::to_string(p->acts_dtype));
    q.elem = p->acts_dtype;
    q.pad_T = p->pad_T;
    q.pad_S1 = p->pad_S1;
    int64_t acts_rows = q.N;
    if (dyn) {
        // sizes are bounds (plan_device_lengths); nothing more to check on the host
    } else if (q.pad_S1 != 0) {
        if (q.pad_S1 < (int64_t)q.S_max + 1 || q.pad_T < q.T_max)
            return fail(RNNT_STATUS_INVALID_VALUE, "padded layout [B, " + std::to_string(q.pad_T) + ", " +
                                                       std::to_string(q.pad_S1) + ", V] too small for max T " +
                                                       std::to_string(q.T_max) + ", max S " + std::to_string(q.S_max));
        acts_rows = (int64_t)q.B * q.pad_T * q.pad_S1;
    }
    if (p->num_rows >= 0 && p->num_rows != acts_rows)
        return fail(RNNT_STATUS_INVALID_VALUE, "acts has " + std::to_string(p->num_rows) + " rows but the " +
                                                   (q.pad_S1 ? "padded layout needs " : "lattice needs sum_b T_b(S_b+1) = ") +
                                                   std::to_string(acts_rows));
    q.align = p->alignment != nullptr || band;
    Carver c;
    q.off_row = c.take(sizeof(int64_t) * (q.B + 1));
    q.off_col = c.take(sizeof(int64_t) * (q.B + 1));
    q.off_colb = c.take(sizeof(int) * q.cols);
    q.off_den = c.take(sizeof(float) * q.N);
    q.off_lp = c.take(sizeof(Lp) * (q.N + 2 * kLpPad));
    q.off_alpha = c.take(sizeof(double) * q.N);
    q.off_beta = c.take(sizeof(double) * q.N);
    q.off_ll = c.take(sizeof(double) * q.B);
    q.off_llb = c.take(sizeof(double) * q.B);
    // the alignment band after the per-row state, so the state's offsets do not depend on the alignment flag (the
    // C++ manager's band getter rebuilds the band in a workspace that holds the state of an earlier computation)
    q.off_mtmp = q.align ? c.take(sizeof(int) * (q.cols + q.B)) : 0;
    q.off_min = q.align ? c.take(sizeof(int) * q.cols) : 0;
    q.off_max = q.align ? c.take(sizeof(int) * q.cols) : 0;
    q.off_dyn = q.dyn ? c.take(sizeof(DynWords)) : 0;
    // the chase launch's ready flags (mrnnt_chase.hip), one word per column (device lengths: per column of the bound),
    // for problems whose shape can take it -- last, so no other offset depends on it
    if (chase_shape_ok(q)) {
        q.flags_bytes = sizeof(unsigned long long) * (size_t)q.cols;
        q.off_flags = c.take(q.flags_bytes);
    }
    q.total = c.at;
    *pl = q;
    return RNNT_STATUS_SUCCESS;
}

DevProblem make_dev(const mrnnt_problem *p, const Plan &pl, const void *ws) {
    void *w = const_cast<void *>(ws);
    DevProblem d;
    d.acts = p->acts;
    d.labels = p->labels;
    d.label_stride = p->label_stride;
    d.T = p->T_dev;
    d.S = p->S_dev;
    if (p->lattice) {  // caller-provided lattice offsets (mrnnt_lattice_host layout)
        const int64_t *lat = static_cast<const int64_t *>(p->lattice);
        d.row_off = lat;
        d.col_off = lat + pl.B + 1;
        d.col_b = reinterpret_cast<const int *>(lat + 2 * (pl.B + 1));
    } else {
        d.row_off = carve<int64_t>(w, pl.off_row);
        d.col_off = carve<int64_t>(w, pl.off_col);
        d.col_b = carve<int>(w, pl.off_colb);
    }
    d.min_s = pl.align ? carve<int>(w, pl.off_min) : nullptr;
    d.max_s = pl.align ? carve<int>(w, pl.off_max) : nullptr;
    d.B = pl.B;
    d.V = pl.V;
    d.blank = p->blank;
    d.occ_skip = tuning().occ_skip;
    d.num_cols = pl.cols;
    d.num_rows = pl.N;
    d.pad_T = pl.pad_T;
    d.pad_S1 = pl.pad_S1;
    d.scale_stride = p->grad_scale_broadcast ? 0 : 1;
    d.col_mul = 0;  // set per pass by mrnnt_forward / mrnnt_backward (tuning().col_scatter)
    d.den = carve<float>(w, pl.off_den);
    d.lp = carve<Lp>(w, pl.off_lp) + kLpPad;
    d.alpha = carve<double>(w, pl.off_alpha);
    d.beta = carve<double>(w, pl.off_beta);
    d.ll = carve<double>(w, pl.off_ll);
    d.llb = carve<double>(w, pl.off_llb);
    d.dyn = pl.dyn ? carve<DynWords>(w, pl.off_dyn) : nullptr;
    d.steal = 0;
    d.dyn_fused = 0;
    d.s_cap = d.t_cap = d.s1_cap = 0;
    d.scatter_above = INT64_MAX;
    d.status_host = nullptr;
    return d;
}

// A multiplier spreading consecutive column indices over the whole lattice: the first prime >= 0.618 cols
// that does not divide cols (so i -> i * m mod cols is a permutation).
static int64_t scatter_mul(int64_t cols) {
    if (cols < 3) return 0;
    for (int64_t m = std::max<int64_t>(2, (int64_t)(0.6180339887 * (double)cols));; ++m) {
        bool prime = true;
        for (int64_t f = 2; f * f <= m && prime; ++f) prime = (m % f) != 0;
        if (prime && cols % m != 0) return m;
    }
}

int64_t column_order(const Plan &pl, int bit) {
    if (tuning().col_xcd & bit) return -1;
    if (!(tuning().col_scatter & bit)) return 0;
    return pl.dyn ? 1 : scatter_mul(pl.cols);
}

static std::mutex g_status_mu;
static int *g_status_host = nullptr;
static int *g_status_dev = nullptr;

int *process_status_word() {
    std::lock_guard<std::mutex> lk(g_status_mu);
    if (!g_status_host) {
        void *h = nullptr, *d = nullptr;
        if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent) != hipSuccess)
            return nullptr;
        if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
            (void)hipHostFree(h);
            return nullptr;
        }
        std::memset(h, 0, 64);
        g_status_host = static_cast<int *>(h);
        g_status_dev = static_cast<int *>(d);
    }
    return g_status_host;
}

RNNTStatus status_device_ptr(const mrnnt_problem *p, int **dev) {
    *dev = nullptr;
    if (!p->status_host) return RNNT_STATUS_SUCCESS;
    {
        std::lock_guard<std::mutex> lk(g_status_mu);
        if (p->status_host == g_status_host) {
            *dev = g_status_dev;
            return RNNT_STATUS_SUCCESS;
        }
    }
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, p->status_host, 0) != hipSuccess || !d)
        return fail(RNNT_STATUS_INVALID_VALUE, "status_host is not host-mapped memory (use mrnnt_status_word())");
    *dev = static_cast<int *>(d);
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus prepare_lattice(const mrnnt_problem *p, const Plan &pl, const DevProblem &d, void *ws,
                           const LatticeOpts &o, hipStream_t stream) {
    const auto run = [&](int id, auto &&launch) { return o.timed ? timed(id, stream, launch) : launch(); };
    int64_t *row_off = carve<int64_t>(ws, pl.off_row), *col_off = carve<int64_t>(ws, pl.off_col);
    int *col_b = carve<int>(ws, pl.off_colb);
    hipError_t e = hipSuccess;
    if (pl.dyn) {  // device-resident lengths: offsets, column map and validation in one launch, no read-back
        DynSetupArgs a;
        std::memset(&a, 0, sizeof(a));
        if (o.report_status) {
            const RNNTStatus st = status_device_ptr(p, &a.status_host);
            if (st != RNNT_STATUS_SUCCESS) return st;
        }
        a.T = p->T_dev;
        a.S = p->S_dev;
        a.B = pl.B;
        a.packed = pl.pad_S1 == 0;
        a.rows = pl.N;
        a.cols_cap = pl.cols;
        a.S_cap = pl.S_max;
        a.T_cap = o.t_cap;  // T_b <= the tightest of the entry point's bound, pad_T and the alignment row stride
        for (const int64_t cap : {pl.pad_S1 ? pl.pad_T : 0, p->alignment ? p->align_stride : 0})
            if (cap) a.T_cap = a.T_cap ? std::min(a.T_cap, cap) : cap;
        a.S1_cap = pl.pad_S1;
        a.scatter_above = o.scatter_above;
        a.row_off = row_off;
        a.col_off = col_off;
        a.col_b = col_b;
        a.lp = o.zero_lp_pads ? d.lp : nullptr;
        a.dyn = d.dyn;
        e = run(K_SETUP, [&] { return launch_setup_dyn(a, stream); });
        if (e != hipSuccess) return fail_hip(e, "device-lengths setup kernel");
    } else if (!p->lattice) {  // lattice offsets on the device (the log-softmax kernel zeroes the lp pads)
        e = run(K_SETUP,
                [&] { return launch_setup(p->T_dev, p->S_dev, pl.B, row_off, col_off, col_b, nullptr, 0, stream); });
        if (e != hipSuccess) return fail_hip(e, "setup kernel");
    }
    if (pl.align && p->alignment) {  // (a plan with band arrays of its own: their owner fills them)
        e = run(K_BAND, [&] {
            return launch_align(d, p->alignment, p->align_stride, p->align_blank, p->max_shift,
                                carve<int>(ws, pl.off_mtmp), carve<int>(ws, pl.off_min), carve<int>(ws, pl.off_max),
                                stream);
        });
        if (e != hipSuccess) return fail_hip(e, "alignment band kernels");
    }
    return RNNT_STATUS_SUCCESS;
}

int64_t grad_scatter_above(const Plan &pl) {
    return ((tuning().col_scatter & 3) != 0 && !(tuning().col_xcd & 3))
               ? (int64_t)streaming_grid(pl.cols, tuning().grad_grid_per_cu)
               : INT64_MAX;
}

RNNTStatus check_row_stride(const char *what, int64_t stride, const char *of, int64_t need, bool dyn, int least) {
    if (stride >= least && (dyn || stride >= need)) return RNNT_STATUS_SUCCESS;
    return fail(RNNT_STATUS_INVALID_VALUE, std::string(what) + " row stride " + std::to_string(stride) + " < max " + of +
                                               " length " + std::to_string(dyn ? (int64_t)least : need));
}

// device lengths, one workgroup per column wanted: workgroups per CU of the grid that hands the columns out instead
constexpr int kStealGridPerCU = 16;

RNNTStatus softmax_pass(const Plan &pl, const DevProblem &d, hipStream_t stream) {
    int grid = streaming_grid(pl.cols, tuning().softmax_grid_per_cu);
    DevProblem ds = d;  // the log-softmax launch's view
    ds.col_mul = column_order(pl, 1);
    if (pl.dyn && tuning().softmax_grid_per_cu <= 0) {  // one workgroup per column needs the column count
        grid = streaming_grid(pl.cols, kStealGridPerCU);
        ds.steal = grid < pl.cols;
    }
    const hipError_t e = timed(K_SOFTMAX, stream, [&] { return launch_softmax(ds, pl.elem, grid, stream); });
    return e == hipSuccess ? RNNT_STATUS_SUCCESS : fail_hip(e, "log-softmax kernel");
}

RNNTStatus posterior_readout(const Plan &pl, const DevProblem &d, const PosteriorArgs &a, hipStream_t stream) {
    const int grid = streaming_grid((pl.cols + 15) / 16, 8);  // column workgroups: 16 waves, one column per wave
    const hipError_t e = timed(K_DP, stream, [&] { return launch_posteriors(d, a, grid, stream); });
    return e == hipSuccess ? RNNT_STATUS_SUCCESS : fail_hip(e, "posterior kernel");
}

RNNTStatus sample_readout(const mrnnt_problem *p, const Plan &pl, const void *ws, int num_samples, uint64_t seed,
                          int64_t first_sample, int *alignments_dev, int64_t out_stride, float *path_costs_dev,
                          hipStream_t stream) {
    if (num_samples < 1)
        return fail(RNNT_STATUS_INVALID_VALUE, "num_samples must be >= 1, got " + std::to_string(num_samples));
    if (first_sample < 0 || first_sample + (int64_t)num_samples > ((int64_t)1 << 32))
        return fail(RNNT_STATUS_INVALID_VALUE, "sample indices [first_sample, first_sample + num_samples) = [" +
                                                   std::to_string(first_sample) + ", " +
                                                   std::to_string(first_sample + (int64_t)num_samples) +
                                                   ") must lie in [0, 2^32]");
    if (!alignments_dev) return fail(RNNT_STATUS_INVALID_VALUE, "alignments is null");
    // with device lengths the kernel bounds every write by the stride instead (and raises the status word)
    RNNTStatus st = check_row_stride("alignments", out_stride, "input", pl.T_max, pl.dyn, 1);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (!ws) return fail(RNNT_STATUS_INVALID_VALUE, "workspace is null");
    if (!p->T_dev || !p->S_dev) return fail(RNNT_STATUS_INVALID_VALUE, "device lengths are required");
    if (!p->labels) return fail(RNNT_STATUS_INVALID_VALUE, "labels is null");
    DevProblem d = make_dev(p, pl, ws);  // acts are never read
    if (pl.dyn && (st = status_device_ptr(p, &d.status_host)) != RNNT_STATUS_SUCCESS) return st;
    const SampleArgs a{alignments_dev, out_stride, path_costs_dev, num_samples, first_sample, seed};
    const hipError_t e = timed(K_DP, stream, [&] { return launch_sample(d, a, stream); });
    if (e != hipSuccess) return fail_hip(e, "sample kernel");
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus check_paths(const Plan &pl, const int *alignments_dev, int64_t path_stride) {
    if (!alignments_dev) return fail(RNNT_STATUS_INVALID_VALUE, "alignments is null");
    // with device lengths T_b <= path_stride joins the device validation
    return check_row_stride("alignments", path_stride, "input", pl.T_max, pl.dyn, 1);
}

PathArgs path_args(void *ws, size_t off_valid, size_t off_carry, size_t off_min, size_t off_max,
                   const int *alignments_dev, int num_paths, int64_t path_stride) {
    PathArgs a;
    a.al = alignments_dev;
    a.stride = path_stride;
    a.K = num_paths;
    a.valid = carve<int>(ws, off_valid);
    a.carry = carve<int>(ws, off_carry);
    a.min_s = carve<int>(ws, off_min);
    a.max_s = carve<int>(ws, off_max);
    a.costs = nullptr;
    a.w = nullptr;
    return a;
}

int64_t inband_rows(int T, int S) {
    int64_t n = 0;
    for (int t = 0; t < T; ++t) n += std::min(t, S) - std::max(0, t - (T - S)) + 1;
    return n;
}

void ExpectState::carve_from(Carver *c, const Plan &pl) {
    off_A = c->take(sizeof(double) * (size_t)pl.N);
    off_Bk = c->take(sizeof(double) * (size_t)pl.N);
    off_R = c->take(sizeof(double) * (size_t)pl.B);
}

void ExpectState::bind(DevProblem *d, void *ws, const float *blank_cost_dev, const float *label_cost_dev) const {
    d->ex_A = carve<double>(ws, off_A);
    d->ex_Bk = carve<double>(ws, off_Bk);
    d->ex_R = carve<double>(ws, off_R);
    d->ex_wb = blank_cost_dev;
    d->ex_we = label_cost_dev;
}

RNNTStatus check_grid(const Plan &pl, bool given, const char *noun, int64_t grid_T, int64_t grid_S1) {
    if (given && (grid_T < pl.T_max || grid_S1 < (int64_t)pl.S_max + 1))
        return fail(RNNT_STATUS_INVALID_VALUE, std::string(noun) + " grid [" + std::to_string(grid_T) + ", " +
                                                   std::to_string(grid_S1) + "] smaller than [max T, max S + 1] = [" +
                                                   std::to_string(pl.T_max) + ", " + std::to_string(pl.S_max + 1) + "]");
    return RNNT_STATUS_SUCCESS;
}

// ---- profiling ---------------------------------------------------------------------------------

static std::mutex g_prof_mu;
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;
// events are created ahead (mrnnt_profile_enable) and recycled, so a timed launch adds two event records and
// no hipEventCreate to the host path it measures (that matters for 0.1 ms steps)
static std::vector<hipEvent_t> g_event_pool;
constexpr size_t kEventPrealloc = 2048;

// timing-only events: no system-scope fence at record (a cache writeback + invalidate between the timed kernels
// would slow the launches being measured)
static hipError_t make_timing_event(hipEvent_t *e) { return hipEventCreateWithFlags(e, hipEventDisableSystemFence); }

static hipEvent_t pooled_event() {  // g_prof_mu held
    if (!g_event_pool.empty()) {
        const hipEvent_t e = g_event_pool.back();
        g_event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    return make_timing_event(&e) == hipSuccess ? e : nullptr;
}

bool profile_begin(int id, hipStream_t s, ProfRec *r) {
    *r = ProfRec{id, nullptr, nullptr};
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        if (!g_prof_on) return false;
        r->a = pooled_event();
        r->b = pooled_event();
        if (!r->a || !r->b) {
            if (r->a) g_event_pool.push_back(r->a);
            if (r->b) g_event_pool.push_back(r->b);
            return false;
        }
    }
    (void)hipEventRecord(r->a, s);
    return true;
}

void profile_end(const ProfRec &r, hipStream_t s) {
    (void)hipEventRecord(r.b, s);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.push_back(r);
}

}  // namespace mrnnt

using namespace mrnnt;

extern "C" {

void mrnnt_profile_enable(int enable) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto &r : g_prof) {  // recycled: a record still pending is complete before the event is recorded again
        g_event_pool.push_back(r.a);
        g_event_pool.push_back(r.b);
    }
    g_prof.clear();
    g_prof_on = enable != 0;
    while (g_prof_on && g_event_pool.size() < kEventPrealloc) {
        hipEvent_t e = nullptr;
        if (make_timing_event(&e) != hipSuccess) break;
        g_event_pool.push_back(e);
    }
}

int mrnnt_profile_read(double *total_ms, int64_t *launches, int n) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (int i = 0; i < n; ++i) {
        if (total_ms) total_ms[i] = 0.0;
        if (launches) launches[i] = 0;
    }
    int bad = 0;
    for (auto &r : g_prof) {
        if (hipEventSynchronize(r.b) != hipSuccess) {
            ++bad;
            continue;
        }
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) {
            ++bad;
            continue;
        }
        if (r.id < n) {
            if (total_ms) total_ms[r.id] += ms;
            if (launches) launches[r.id] += 1;
        }
    }
    return bad;
}

}  // extern "C"
