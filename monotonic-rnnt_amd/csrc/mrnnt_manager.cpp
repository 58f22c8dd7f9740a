// mrnnt_manager.cpp -- the reference-shaped C++ surface of libmonotonic_rnnt_amd.so: GpuRNNTWorkspaceManager<float>,
// GpuRNNTComputer<float> and compute_rnnt_loss for RNNT_GPU (reference gpu_workspace_manager.h, gpu_rnnt.h,
// src/rnnt_entrypoint.cpp), on top of the flat ABI (mrnnt_capi.cpp). This surface synchronises, as its contract
// returns host costs (gpu_rnnt.h:229); of the internals it uses make_plan, make_dev and launch_state_f32 alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#pragma GCC visibility push(default)
#include "cpu_rnnt.h"
#include "cpu_workspace_manager.h"
#include "gpu_rnnt.h"
#include "gpu_workspace_manager.h"
#include "mrnnt.h"
#include "rnnt_entrypoint.h"
#pragma GCC visibility pop
#include "mrnnt_plan.h"

using namespace mrnnt;

struct mrnnt_gpu_ws_state {
    const float *acts;
    const int *labels;
    int B, V;
    const int *T_dev;
    const int *S_dev;
    void *workspace = nullptr;
    bool owned = false;
    const int *alignment = nullptr;
    int max_shift = 0;
    int align_blank = 0;
    // the last computation on the workspace (what the inspection getters read back)
    bool computed = false;
    bool with_beta = false;
    int blank = 0;
    hipStream_t stream = nullptr;
};

namespace {

// Host copies of T/S (the reference makes the same D2H copies, gpu_workspace_manager.h:87-96), ordered on `stream`.
bool host_lengths(const mrnnt_gpu_ws_state *s, std::vector<int> &T, std::vector<int> &S, hipStream_t stream = nullptr) {
    T.assign(s->B, 0);
    S.assign(s->B, 0);
    if (s->B <= 0) return true;
    if (hipMemcpyAsync(T.data(), s->T_dev, sizeof(int) * s->B, hipMemcpyDeviceToHost, stream) != hipSuccess) return false;
    if (hipMemcpyAsync(S.data(), s->S_dev, sizeof(int) * s->B, hipMemcpyDeviceToHost, stream) != hipSuccess) return false;
    return hipStreamSynchronize(stream) == hipSuccess;
}

// (T, S) on the host, ordered on the stream of the last computation; zeros where the copy fails
struct Lengths {
    std::vector<int> T, S;
};
Lengths lengths_of(const mrnnt_gpu_ws_state *s) {
    Lengths ts;
    (void)host_lengths(s, ts.T, ts.S, s->stream);
    return ts;
}

int max_of(const std::vector<int> &v) { return v.empty() ? 0 : *std::max_element(v.begin(), v.end()); }

mrnnt_problem problem_of(const mrnnt_gpu_ws_state *s, const std::vector<int> &T, const std::vector<int> &S,
                         int blank) {
    mrnnt_problem p;
    std::memset(&p, 0, sizeof(p));
    p.B = s->B;
    p.V = s->V;
    p.blank = blank;
    p.T_host = T.data();
    p.S_host = S.data();
    p.T_dev = s->T_dev;
    p.S_dev = s->S_dev;
    p.acts = s->acts;
    p.labels = s->labels;
    // reference quirks kept on this surface: label row stride = max(S) (gpu_rnnt_kernel.h:133),
    // alignment row stride = max(T) (gpu_workspace_manager.h:200)
    p.label_stride = max_of(S);
    p.alignment = s->alignment;
    p.align_stride = max_of(T);
    p.align_blank = s->align_blank;
    p.max_shift = s->max_shift;
    p.num_rows = -1;
    return p;
}

// Row offset of each utterance in the reference's dense T*(S+1) order (its int offsets), and the rows in all.
std::vector<int> row_offsets(const std::vector<int> &T, const std::vector<int> &S, int64_t *rows = nullptr) {
    std::vector<int> off(T.size(), 0);
    int64_t r = 0;
    for (size_t b = 0; b < T.size(); ++b) {
        off[b] = (int)r;
        r += (int64_t)T[b] * (S[b] + 1);
    }
    if (rows) *rows = r;
    return off;
}

// The reference manager's public view (gpu_workspace_manager.h:58-85, laid out in its order, :228-254, 301-346).
struct RefView {
    size_t denom, alphas, betas, dsi, vso, llf, llb, B, V, Smax, Tmax, mn, mx, total;
};

RefView ref_view_layout(int B, int64_t N, int T_max) {
    RefView v;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += bytes;
        return at;
    };
    v.denom = take(sizeof(float) * N);
    v.alphas = take(sizeof(float) * N);
    v.betas = take(sizeof(float) * N);
    v.dsi = take(sizeof(int) * B);
    v.vso = take(sizeof(int) * B);
    v.llf = take(sizeof(float) * B);
    v.llb = take(sizeof(float) * B);
    v.B = take(sizeof(int));
    v.V = take(sizeof(int));
    v.Smax = take(sizeof(int));
    v.Tmax = take(sizeof(int));
    v.mn = take(sizeof(int) * (size_t)B * T_max);
    v.mx = take(sizeof(int) * (size_t)B * T_max);
    v.total = o;
    return v;
}

// The manager's workspace = the flat plan + B device floats for the costs + the reference's view. The view's offset
// is fixed by the larger of the plans with and without an alignment (restrict_to_alignment may come after
// set_workspace); the costs follow the plan of the current call.
RNNTStatus manager_size(const mrnnt_gpu_ws_state *s, const std::vector<int> &T, const std::vector<int> &S,
                        size_t *bytes, size_t *costs_off, size_t *view_off = nullptr) {
    mrnnt_problem p = problem_of(s, T, S, 0);
    // size only depends on lengths and the alignment flag; blank range is checked at compute time
    size_t b = 0, b_max = 0;
    RNNTStatus st = mrnnt_workspace_size(&p, &b);
    if (st != RNNT_STATUS_SUCCESS) return st;
    int dummy = 0;
    p.alignment = p.alignment ? p.alignment : &dummy;
    if ((st = mrnnt_workspace_size(&p, &b_max)) != RNNT_STATUS_SUCCESS) return st;
    p.alignment = nullptr;
    size_t b_plain = 0;
    if ((st = mrnnt_workspace_size(&p, &b_plain)) != RNNT_STATUS_SUCCESS) return st;
    b_max = std::max(b_max, b_plain);
    *costs_off = align_up(b);
    const size_t voff = align_up(align_up(b_max) + sizeof(float) * std::max(1, s->B));
    int64_t N = 0;
    row_offsets(T, S, &N);
    *bytes = voff + ref_view_layout(s->B, N, max_of(T)).total;
    if (view_off) *view_off = voff;
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus manager_compute(GpuRNNTWorkspaceManager<float> &wm, int blank, hipStream_t stream, float *costs,
                           float *grads) {
    mrnnt_gpu_ws_state *s = wm.state();
    if (!costs) return fail(RNNT_STATUS_INVALID_VALUE, "costs is null");
    if (!s->workspace) return fail(RNNT_STATUS_INVALID_VALUE, "workspace not set (set_workspace/create_workspace)");
    std::vector<int> T, S;
    if (!host_lengths(s, T, S, stream)) return fail(RNNT_STATUS_MEMOPS_FAILED, "copying lengths to host");
    size_t bytes = 0, coff = 0;
    RNNTStatus st = manager_size(s, T, S, &bytes, &coff);
    if (st != RNNT_STATUS_SUCCESS) return st;
    mrnnt_problem p = problem_of(s, T, S, blank);
    // this surface synchronises anyway (host costs): read the labels back and range-check them, as the flat
    // entry points cannot without a sync (there an out-of-range device label gives a non-finite cost). The copy
    // is ordered on the caller's stream, after whatever produced the labels there.
    if (p.label_stride > 0) {
        std::vector<int> lab((size_t)s->B * p.label_stride);
        if (hipMemcpyAsync(lab.data(), s->labels, sizeof(int) * lab.size(), hipMemcpyDeviceToHost, stream) !=
                hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return fail(RNNT_STATUS_MEMOPS_FAILED, "copying labels to host");
        for (int b = 0; b < s->B; ++b)
            for (int i = 0; i < S[b]; ++i) {
                const int l = lab[(size_t)b * p.label_stride + i];
                if (l < 0 || l >= s->V)
                    return fail(RNNT_STATUS_INVALID_VALUE, "label " + std::to_string(l) + " at (" + std::to_string(b) +
                                                               ", " + std::to_string(i) + ") outside [0, V)");
            }
    }
    float *costs_dev = carve<float>(s->workspace, coff);
    st = mrnnt_cost_and_grad(&p, s->workspace, coff, costs_dev, grads, nullptr, stream);
    if (st != RNNT_STATUS_SUCCESS) return st;
    s->computed = true;
    s->with_beta = grads != nullptr;
    s->blank = blank;
    s->stream = stream;
    // the reference's public members: the view of this computation (betas / ll_backward only with the gradient, as
    // the reference's cost() skips the beta pass)
    if (wm.denom) {
        Plan pl;
        if ((st = make_plan(&p, &pl)) != RNNT_STATUS_SUCCESS) return st;
        const DevProblem d = make_dev(&p, pl, s->workspace);
        if ((st = mrnnt_read_denoms(&p, s->workspace, wm.denom, stream)) != RNNT_STATUS_SUCCESS) return st;
        hipError_t ev = launch_state_f32(d, wm.alphas, grads ? wm.betas : nullptr, wm.ll_forward,
                                         grads ? wm.ll_backward : nullptr, stream);
        if (ev != hipSuccess) return fail_hip(ev, "reference view kernel");
        st = mrnnt_read_band(&p, s->workspace, wm.min_allowed_s, wm.max_allowed_s, max_of(T), stream);
        if (st != RNNT_STATUS_SUCCESS) return st;
    }
    hipError_t e = hipMemcpyAsync(costs, costs_dev, sizeof(float) * s->B, hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return fail(RNNT_STATUS_MEMOPS_FAILED, std::string("costs D2H: ") + hipGetErrorString(e));
    e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail_hip(e, "stream synchronize");
    return RNNT_STATUS_SUCCESS;
}

// A device scratch buffer for the inspection getters (they are synchronous, as the reference's are).
struct DevBuf {
    void *p = nullptr;
    explicit DevBuf(size_t bytes) {
        if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) p = nullptr;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
};

// No view: the reference's public members before set_workspace / after free_workspace.
void clear_view(GpuRNNTWorkspaceManager<float> &wm) {
    wm.denom = wm.alphas = wm.betas = wm.ll_forward = wm.ll_backward = nullptr;
    wm.B = wm.V = wm.S_max = wm.T_max = wm.min_allowed_s = wm.max_allowed_s = wm.denom_start_indices =
        wm.var_start_offsets = nullptr;
}

int64_t band_ld(const mrnnt_problem &p) { return std::max<int64_t>(1, p.align_stride); }

// A state getter (they are synchronous, as the reference's are): host copies of the lengths, the problem of the last
// computation on the workspace, and one element per lattice row, per utterance or per band entry [B, band_ld] that
// `read` fills on the device as In, returned as Out. Empty on failure or when there is no workspace.
enum Extent { PER_ROW, PER_UTT, PER_BAND };
template <class In, class Out, class F>
std::vector<Out> get_state(const mrnnt_gpu_ws_state *s, Extent ext, F &&read) {
    std::vector<int> T, S;
    if (!host_lengths(s, T, S, s->stream) || !s->workspace) return {};
    const mrnnt_problem p = problem_of(s, T, S, s->blank);
    int64_t rows = 0;
    row_offsets(T, S, &rows);
    const size_t n = ext == PER_ROW ? (size_t)(int)rows : (size_t)s->B * (ext == PER_BAND ? band_ld(p) : 1);
    DevBuf buf(sizeof(In) * n);
    if (!buf.p || read(p, static_cast<In *>(buf.p)) != RNNT_STATUS_SUCCESS) return {};
    std::vector<In> h(n);
    if (n && (hipMemcpyAsync(h.data(), buf.p, sizeof(In) * n, hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
              hipStreamSynchronize(s->stream) != hipSuccess))
        return {};
    return std::vector<Out>(h.begin(), h.end());
}

}  // namespace

GpuRNNTWorkspaceManager<float>::GpuRNNTWorkspaceManager(const float *const acts_, const int *const labels_,
                                                        const int B_, const int *T_, const int *S_, const int V_)
    : st_(new mrnnt_gpu_ws_state),
      workspace_(nullptr),
      B_h(B_),
      V_h(V_),
      T(T_),
      S(S_),
      acts(acts_),
      labels(labels_) {
    clear_view(*this);
    st_->acts = acts_;
    st_->labels = labels_;
    st_->B = B_;
    st_->V = V_;
    st_->T_dev = T_;
    st_->S_dev = S_;
}

GpuRNNTWorkspaceManager<float>::~GpuRNNTWorkspaceManager() { delete st_; }

RNNTStatus GpuRNNTWorkspaceManager<float>::get_workspace_size(size_t *size_bytes) const {
    if (st_->B <= 0) return fail(RNNT_STATUS_INVALID_VALUE, "B must be > 0");
    std::vector<int> Th, Sh;
    if (!host_lengths(st_, Th, Sh)) return fail(RNNT_STATUS_MEMOPS_FAILED, "copying lengths to host");
    size_t coff = 0;
    // alignment may be registered later: manager_size sizes the view for either layout
    return manager_size(st_, Th, Sh, size_bytes, &coff);
}

// (reference :256-329) the public members point into the workspace's view region; the constants and the default band
// are uploaded with blocking copies, as the reference's cudaMemcpy calls do
void GpuRNNTWorkspaceManager<float>::set_workspace(void *workspace) {
    if (st_->owned && st_->workspace && st_->workspace != workspace) (void)hipFree(st_->workspace);
    st_->workspace = workspace;
    st_->owned = false;
    st_->computed = false;
    workspace_ = workspace;
    clear_view(*this);
    std::vector<int> Th, Sh;
    size_t bytes = 0, coff = 0, voff = 0;
    if (!workspace || st_->B <= 0 || !host_lengths(st_, Th, Sh) ||
        manager_size(st_, Th, Sh, &bytes, &coff, &voff) != RNNT_STATUS_SUCCESS)
        return;
    int64_t N = 0;
    const std::vector<int> off = row_offsets(Th, Sh, &N);
    const int Tm = max_of(Th), Sm = max_of(Sh);
    const RefView v = ref_view_layout(st_->B, N, Tm);
    void *base = carve<char>(workspace, voff);
    denom = carve<float>(base, v.denom);
    alphas = carve<float>(base, v.alphas);
    betas = carve<float>(base, v.betas);
    denom_start_indices = carve<int>(base, v.dsi);
    var_start_offsets = carve<int>(base, v.vso);
    ll_forward = carve<float>(base, v.llf);
    ll_backward = carve<float>(base, v.llb);
    B = carve<int>(base, v.B);
    V = carve<int>(base, v.V);
    S_max = carve<int>(base, v.Smax);
    T_max = carve<int>(base, v.Tmax);
    min_allowed_s = carve<int>(base, v.mn);
    max_allowed_s = carve<int>(base, v.mx);
    std::vector<int> mn((size_t)st_->B * Tm, 0), mx((size_t)st_->B * Tm);
    for (int b = 0; b < st_->B; ++b) std::fill_n(mx.begin() + (size_t)b * Tm, Tm, Sh[b]);
    const int consts[4] = {st_->B, st_->V, Sm, Tm};
    bool ok = hipMemcpy(denom_start_indices, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(var_start_offsets, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(B, consts, sizeof(consts), hipMemcpyHostToDevice) == hipSuccess;  // B, V, S_max, T_max
    ok = ok && hipMemcpy(min_allowed_s, mn.data(), sizeof(int) * mn.size(), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(max_allowed_s, mx.data(), sizeof(int) * mx.size(), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) (void)fail(RNNT_STATUS_MEMOPS_FAILED, "set_workspace: uploading the reference view's constants");
}

RNNTStatus GpuRNNTWorkspaceManager<float>::create_workspace() {
    size_t bytes = 0;
    const RNNTStatus st = get_workspace_size(&bytes);
    if (st != RNNT_STATUS_SUCCESS) return st;
    void *w = nullptr;
    if (hipMalloc(&w, bytes) != hipSuccess) return fail(RNNT_STATUS_MEMOPS_FAILED, "hipMalloc workspace");
    set_workspace(w);
    st_->owned = true;
    return RNNT_STATUS_SUCCESS;
}

void GpuRNNTWorkspaceManager<float>::free_workspace() {
    if (st_->workspace) (void)hipFree(st_->workspace);
    st_->workspace = nullptr;
    st_->owned = false;
    st_->computed = false;
    workspace_ = nullptr;
    clear_view(*this);
}

void GpuRNNTWorkspaceManager<float>::restrict_to_alignment(const int *const alignments, int max_shift, int blank_idx) {
    st_->alignment = alignments;
    st_->max_shift = max_shift;
    st_->align_blank = blank_idx;
}

int GpuRNNTWorkspaceManager<float>::B_host() const { return st_->B; }
int GpuRNNTWorkspaceManager<float>::V_host() const { return st_->V; }

std::vector<int> GpuRNNTWorkspaceManager<float>::T_host() const { return lengths_of(st_).T; }
std::vector<int> GpuRNNTWorkspaceManager<float>::S_host() const { return lengths_of(st_).S; }

int GpuRNNTWorkspaceManager<float>::num_denoms() const {
    const Lengths ts = lengths_of(st_);
    int64_t n = 0;
    row_offsets(ts.T, ts.S, &n);
    return (int)n;
}

int GpuRNNTWorkspaceManager<float>::num_fwd_bwd_var_positions() const { return num_denoms(); }

std::vector<int> GpuRNNTWorkspaceManager<float>::var_start_offsets_host() const {
    const Lengths ts = lengths_of(st_);
    return row_offsets(ts.T, ts.S);
}

int GpuRNNTWorkspaceManager<float>::S_max_host() const { return max_of(S_host()); }
int GpuRNNTWorkspaceManager<float>::T_max_host() const { return max_of(T_host()); }

std::vector<float> GpuRNNTWorkspaceManager<float>::acts_host() const {
    const size_t n = (size_t)num_denoms() * (size_t)std::max(0, st_->V);
    std::vector<float> h(n);
    if (n && (hipMemcpyAsync(h.data(), st_->acts, sizeof(float) * n, hipMemcpyDeviceToHost, st_->stream) != hipSuccess ||
              hipStreamSynchronize(st_->stream) != hipSuccess))
        return {};
    return h;
}

// The getters below read the state of the last cost / cost_and_grad on this workspace through the flat
// inspection entry points (mrnnt_read_denoms / _state / _loglik / _band), in the reference's dense T*(S+1)
// per-utterance order (var_start_offsets[b] + t*(S_b+1) + s).
std::vector<float> GpuRNNTWorkspaceManager<float>::denom_host() const {
    return get_state<float, float>(st_, PER_ROW, [&](const mrnnt_problem &p, float *d) {
        return mrnnt_read_denoms(&p, st_->workspace, d, st_->stream);
    });
}

std::vector<float> GpuRNNTWorkspaceManager<float>::alphas_host() const {
    return get_state<double, float>(st_, PER_ROW, [&](const mrnnt_problem &p, double *d) {
        return mrnnt_read_state(&p, st_->workspace, nullptr, d, nullptr, st_->stream);
    });
}

std::vector<float> GpuRNNTWorkspaceManager<float>::betas_host() const {
    return get_state<double, float>(st_, PER_ROW, [&](const mrnnt_problem &p, double *d) {
        return mrnnt_read_state(&p, st_->workspace, nullptr, nullptr, d, st_->stream);
    });
}

std::vector<float> GpuRNNTWorkspaceManager<float>::ll_forward_host() const {
    return get_state<double, float>(st_, PER_UTT, [&](const mrnnt_problem &p, double *d) {
        return mrnnt_read_loglik(&p, st_->workspace, d, nullptr, st_->stream);
    });
}

std::vector<float> GpuRNNTWorkspaceManager<float>::ll_backward_host() const {
    return get_state<double, float>(st_, PER_UTT, [&](const mrnnt_problem &p, double *d) {
        return mrnnt_read_loglik(&p, st_->workspace, nullptr, d, st_->stream);
    });
}

std::vector<int> GpuRNNTWorkspaceManager<float>::min_allowed_s_host() const {
    return get_state<int, int>(st_, PER_BAND, [&](const mrnnt_problem &p, int *d) {
        return mrnnt_read_band(&p, st_->workspace, d, nullptr, band_ld(p), st_->stream);
    });
}

std::vector<int> GpuRNNTWorkspaceManager<float>::max_allowed_s_host() const {
    return get_state<int, int>(st_, PER_BAND, [&](const mrnnt_problem &p, int *d) {
        return mrnnt_read_band(&p, st_->workspace, nullptr, d, band_ld(p), st_->stream);
    });
}

GpuRNNTComputer<float>::GpuRNNTComputer(GpuRNNTWorkspaceManager<float> &workspace_manager, int blank,
                                        hipStream_t stream)
    : workspace_manager_(workspace_manager), blank_(blank), stream_(stream) {}

RNNTStatus GpuRNNTComputer<float>::cost_and_grad(float *costs, float *grads) {
    return manager_compute(workspace_manager_, blank_, stream_, costs, grads);
}

RNNTStatus GpuRNNTComputer<float>::cost(float *costs) {
    return manager_compute(workspace_manager_, blank_, stream_, costs, nullptr);
}

// compute_rnnt_loss (mrnnt_entry.cpp) for loc = RNNT_GPU
RNNTStatus mrnnt::gpu_compute_rnnt_loss(RNNTWorkspaceManager &workspace_manager, RNNTOptions options, float *costs,
                                        float *gradients) {
    auto *gm = dynamic_cast<GpuRNNTWorkspaceManager<float> *>(&workspace_manager);
    if (!gm) return fail(RNNT_STATUS_INVALID_VALUE, "workspace manager is not a GpuRNNTWorkspaceManager<float>");
    GpuRNNTComputer<float> computer(*gm, options.blank_label, options.stream);
    return gradients != nullptr ? computer.cost_and_grad(costs, gradients) : computer.cost(costs);
}
