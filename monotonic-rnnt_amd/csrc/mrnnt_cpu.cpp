// mrnnt_cpu.cpp -- the host (RNNT_CPU) implementation of libmonotonic_rnnt_amd.so: the flat C entry points
// mrnnt_cpu_* (include/mrnnt.h), CpuRNNTWorkspaceManager<float> (include/cpu_workspace_manager.h) and
// CpuRNNTComputer<float> (include/cpu_rnnt.h). It serves the reference's CPU surface
// (src/rnnt_entrypoint.cpp:22-31, pytorch_binding/monotonic_rnnt.cu:16-77) with the GPU path's semantics.
//
// Same three passes as the HIP path, laid out for a multicore host instead of a port of cpu_rnnt.h:
//   1. log-softmax row reduce over the in-band (or alignment-window) rows, OpenMP over lattice columns,
//      SIMD max / exp-sum (fp32 lanes, fp64 block totals) -> den, lpb = z[blank] + den, lpe = z[label] + den
//      (the reference: OpenMP over utterances only and a serial log_sum_exp per element, cpu_rnnt.h:96-111)
//   2. alpha / beta recursion per utterance in fp64 (cpu_rnnt.h:140-214 semantics, rnnt_helper.h:16-30 LSE),
//      OpenMP over utterances x direction
//   3. logit gradient, OpenMP over lattice columns, SIMD exp, dL/dcost fused, rows whose occupancy is below
//      e^-110 written as exact zeros without reading acts (cpu_rnnt.h:216-249 formula)
// Offsets are 64-bit throughout (the reference's int act_index overflows past 2^31 elements).
// The hot row loops are compiled three times (AVX-512 / AVX2+FMA / baseline x86-64) and picked at load
// time by the CPU's features (GCC function multiversioning).
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#pragma GCC visibility push(default)
#include "cpu_rnnt.h"
#include "cpu_workspace_manager.h"
#include "mrnnt.h"
#pragma GCC visibility pop
#include "mrnnt_host.h"
#include "mrnnt_sample.h"

using mrnnt::set_error;

namespace {

constexpr double kNegInf = -std::numeric_limits<double>::infinity();

// the loss gradient's flush-dead rule (LossRows::row): always on in the product; the development build can switch it
// off (mrnnt_cpu_flush_rows) to show that the gradient's bits do not depend on it
#ifdef MRNNT_DEVTOOLS
int g_flush_rows = 1;
#else
constexpr int g_flush_rows = 1;
#endif

// ---- SIMD row kernels ---------------------------------------------------------------------------------

// e^x in fp32 from plain arithmetic (so the loops vectorise): Cody-Waite reduction by ln 2, degree-6
// polynomial on |r| <= ln2/2 (relative error ~2e-7), exponent assembled in the bits. Results below
// e^-87 (< 1.7e-38, the fp32 normal range) flush to 0; x > 88.7 gives +inf; NaN propagates.
static inline __attribute__((always_inline)) float vexp(float x) {
    constexpr float kMagic = 12582912.0f;  // 1.5 * 2^23: adding it rounds to an integer in the low bits
    const float xc = std::min(std::max(x, -87.0f), 88.7f);
    const float tq = xc * 1.44269504088896341f + kMagic;
    // the integer part in unsigned arithmetic: NaN input makes tq NaN and n garbage (the result is replaced below),
    // which in signed arithmetic was an overflow / negative left shift (UBSan, `make asan`)
    const unsigned n = __builtin_bit_cast(unsigned, tq) - __builtin_bit_cast(unsigned, kMagic);
    const float fn = tq - kMagic;
    float r = xc - fn * 0.693145751953125f;
    r = r - fn * 1.428606765330187045e-06f;
    const float p =
        1.0f + r * (1.0f + r * (0.5f + r * (0.166666672f + r * (0.0416666418f + r * (0.00833345205f +
                                                                                     r * 0.00138888808f)))));
    float res = p * __builtin_bit_cast(float, (n + 127u) << 23);
    res = (x < -87.0f) ? 0.0f : res;
    res = (x > 88.7f) ? std::numeric_limits<float>::infinity() : res;
    return (x != x) ? x : res;
}

constexpr int kBlock = 512;  // elements per fp32 partial-sum block (then accumulated in fp64)

// max and sum_v e^(z_v - max) of one row; NaN elements are skipped by the max and poison the sum
static inline __attribute__((always_inline)) void row_max_sum_body(const float *__restrict__ z, int V, float &m_out,
                                                                   double &sum_out) {
    float m = -std::numeric_limits<float>::infinity();
#pragma omp simd reduction(max : m)
    for (int v = 0; v < V; ++v) m = z[v] > m ? z[v] : m;
    double sum = 0.0;
    for (int v0 = 0; v0 < V; v0 += kBlock) {
        const int v1 = std::min(V, v0 + kBlock);
        float s = 0.0f;
#pragma omp simd reduction(+ : s)
        for (int v = v0; v < v1; ++v) s += vexp(z[v] - m);
        sum += (double)s;
    }
    m_out = m;
    sum_out = sum;
}

// The same over the row without element `skip` (the factorised blank, hat_row): max and sum_{v != skip} e^(z_v - max),
// the exps against 0 where every other element is -inf (sum 0, not e^(-inf + inf)); NaN poisons the sum as above.
static inline __attribute__((always_inline)) void row_max_sum_skip_body(const float *__restrict__ z, int V, int skip,
                                                                        float &m_out, double &sum_out) {
    constexpr float ninf = -std::numeric_limits<float>::infinity();
    float m = ninf;
#pragma omp simd reduction(max : m)
    for (int v = 0; v < V; ++v) {
        const float x = v == skip ? ninf : z[v];
        m = x > m ? x : m;
    }
    const float mr = m == ninf ? 0.0f : m;
    double sum = 0.0;
    for (int v0 = 0; v0 < V; v0 += kBlock) {
        const int v1 = std::min(V, v0 + kBlock);
        float s = 0.0f;
#pragma omp simd reduction(+ : s)
        for (int v = v0; v < v1; ++v) s += v == skip ? 0.0f : vexp(z[v] - mr);
        sum += (double)s;
    }
    m_out = m;
    sum_out = sum;
}

// g_v = e^(z_v + c) * sc (g may be z itself: element-wise, each element read before it is written)
static inline __attribute__((always_inline)) void grad_row_body(const float *z, float *g, int V, float c, float sc) {
#pragma omp simd
    for (int v = 0; v < V; ++v) g[v] = vexp(z[v] + c) * sc;
}

__attribute__((target("default"))) void row_max_sum(const float *z, int V, float &m, double &s) {
    row_max_sum_body(z, V, m, s);
}
__attribute__((target("avx2,fma"))) void row_max_sum(const float *z, int V, float &m, double &s) {
    row_max_sum_body(z, V, m, s);
}
__attribute__((target("avx512f,avx512dq,avx512bw,avx512vl,fma"))) void row_max_sum(const float *z, int V, float &m,
                                                                                    double &s) {
    row_max_sum_body(z, V, m, s);
}

__attribute__((target("default"))) void row_max_sum_skip(const float *z, int V, int skip, float &m, double &s) {
    row_max_sum_skip_body(z, V, skip, m, s);
}
__attribute__((target("avx2,fma"))) void row_max_sum_skip(const float *z, int V, int skip, float &m, double &s) {
    row_max_sum_skip_body(z, V, skip, m, s);
}
__attribute__((target("avx512f,avx512dq,avx512bw,avx512vl,fma"))) void row_max_sum_skip(const float *z, int V, int skip,
                                                                                         float &m, double &s) {
    row_max_sum_skip_body(z, V, skip, m, s);
}

__attribute__((target("default"))) void grad_row(const float *z, float *g, int V, float c, float sc) {
    grad_row_body(z, g, V, c, sc);
}
__attribute__((target("avx2,fma"))) void grad_row(const float *z, float *g, int V, float c, float sc) {
    grad_row_body(z, g, V, c, sc);
}
__attribute__((target("avx512f,avx512dq,avx512bw,avx512vl,fma"))) void grad_row(const float *z, float *g, int V,
                                                                                 float c, float sc) {
    grad_row_body(z, g, V, c, sc);
}

// log(e^x + e^y) with fp64 state (rnnt_helper.h:16-30): one -inf input returns the other exactly, both
// -inf is -inf, NaN propagates (the HIP path's lse2 in mrnnt_device.h has the same cases). fmax drops a NaN
// operand, so the -inf case tests both operands: (NaN, -inf) -- every band-edge cell below a NaN row -- is NaN
// through x - y, not "no path".
inline double lse(double x, double y) {
    const double m = std::fmax(x, y);
    if (x == kNegInf && y == kNegInf) return kNegInf;
    return m + std::log1p(std::exp(-std::fabs(x - y)));
}

// ---- plan --------------------------------------------------------------------------------------------

struct CpuPlan {
    int B = 0, V = 0, S_max = 0, T_max = 0;
    int64_t N = 0, cols = 0, pad_T = 0, pad_S1 = 0;
    bool align = false;
    std::vector<int64_t> row_off, col_off;
    size_t off_den = 0, off_lpb = 0, off_lpe = 0, off_alpha = 0, off_beta = 0, off_ll = 0, off_llb = 0, off_min = 0,
           off_max = 0, total = 0;
};

constexpr size_t kAlign = 64;
size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

// carves aligned workspace arrays one after the other; `at` ends as the total
struct Carver {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t off = at;
        at = align_up(at + bytes);
        return off;
    }
};

// band: the plan holds the band arrays although the problem has no alignment (mrnnt_cpu_path_*: the paths' hull)
RNNTStatus make_cpu_plan(const mrnnt_problem *p, CpuPlan *pl, bool band = false) {
    if (!p) return set_error(RNNT_STATUS_INVALID_VALUE, "null problem");
    if (p->B <= 0) return set_error(RNNT_STATUS_INVALID_VALUE, "B must be > 0");
    if (p->V <= 0) return set_error(RNNT_STATUS_INVALID_VALUE, "V must be > 0");
    if (!p->T_host || !p->S_host) return set_error(RNNT_STATUS_INVALID_VALUE, "host lengths are required");
    if (p->blank < 0 || p->blank >= p->V) return set_error(RNNT_STATUS_INVALID_VALUE, "blank label out of range [0, V)");
    if (p->acts_dtype != MRNNT_F32)
        return set_error(RNNT_STATUS_INVALID_VALUE, "the CPU implementation takes float32 acts only");
    CpuPlan q;
    q.B = p->B;
    q.V = p->V;
    q.row_off.assign(q.B + 1, 0);
    q.col_off.assign(q.B + 1, 0);
    for (int b = 0; b < q.B; ++b) {
        const int T = p->T_host[b], S = p->S_host[b];
        // reference validation: cpu_workspace_manager.h:99-107
        if (T <= 0 || S < 0 || T < S)
            return set_error(RNNT_STATUS_INVALID_VALUE, "invalid lengths at utterance " + std::to_string(b) + ": T=" +
                                                            std::to_string(T) + " S=" + std::to_string(S) +
                                                            " (need T > 0, S >= 0, T >= S)");
        q.row_off[b + 1] = q.row_off[b] + (int64_t)T * (S + 1);
        q.col_off[b + 1] = q.col_off[b] + T;
        q.S_max = std::max(q.S_max, S);
        q.T_max = std::max(q.T_max, T);
    }
    q.N = q.row_off[q.B];
    q.cols = q.col_off[q.B];
    if (q.S_max > 0 && p->label_stride < q.S_max)
        return set_error(RNNT_STATUS_INVALID_VALUE, "label row stride " + std::to_string(p->label_stride) +
                                                        " < max label length " + std::to_string(q.S_max));
    q.align = p->alignment != nullptr || band;
    if (p->alignment && p->align_stride < q.T_max)
        return set_error(RNNT_STATUS_INVALID_VALUE, "alignment row stride " + std::to_string(p->align_stride) +
                                                        " < max input length " + std::to_string(q.T_max));
    q.pad_T = p->pad_T;
    q.pad_S1 = p->pad_S1;
    int64_t acts_rows = q.N;
    if (q.pad_S1 != 0) {
        if (q.pad_S1 < (int64_t)q.S_max + 1 || q.pad_T < q.T_max)
            return set_error(RNNT_STATUS_INVALID_VALUE, "padded layout too small for max T " + std::to_string(q.T_max) +
                                                            ", max S " + std::to_string(q.S_max));
        acts_rows = (int64_t)q.B * q.pad_T * q.pad_S1;
    }
    if (p->num_rows >= 0 && p->num_rows != acts_rows)
        return set_error(RNNT_STATUS_INVALID_VALUE, "acts has " + std::to_string(p->num_rows) + " rows but the " +
                                                        (q.pad_S1 ? "padded layout needs " : "lattice needs sum_b T_b(S_b+1) = ") +
                                                        std::to_string(acts_rows));
    Carver ws;
    q.off_den = ws.take(sizeof(float) * q.N);
    q.off_lpb = ws.take(sizeof(double) * q.N);
    q.off_lpe = ws.take(sizeof(double) * q.N);
    q.off_alpha = ws.take(sizeof(double) * q.N);
    q.off_beta = ws.take(sizeof(double) * q.N);
    q.off_ll = ws.take(sizeof(double) * q.B);
    q.off_llb = ws.take(sizeof(double) * q.B);
    q.off_min = q.align ? ws.take(sizeof(int) * q.cols) : 0;
    q.off_max = q.align ? ws.take(sizeof(int) * q.cols) : 0;
    q.total = ws.at;
    *pl = std::move(q);
    return RNNT_STATUS_SUCCESS;
}

// labels of utterance b (null without labels: every S is 0)
inline const int *utt_labels(const mrnnt_problem *p, int b) {
    return p->labels ? p->labels + (int64_t)b * p->label_stride : nullptr;
}

RNNTStatus check_workspace(const void *ws, size_t ws_bytes, size_t need) {
    if (!ws || ws_bytes < need)
        return set_error(RNNT_STATUS_INVALID_VALUE, "workspace too small: need " + std::to_string(need) + " bytes");
    return RNNT_STATUS_SUCCESS;
}

// the *_workspace_size entry points: the total of the plan that `make` fills
template <class Plan, class F>
RNNTStatus plan_bytes(size_t *bytes, F &&make) {
    if (!bytes) return set_error(RNNT_STATUS_INVALID_VALUE, "null size pointer");
    Plan pl;
    const RNNTStatus st = make(&pl);
    if (st == RNNT_STATUS_SUCCESS) *bytes = pl.total;
    return st;
}

RNNTStatus check_inputs(const mrnnt_problem *p, const CpuPlan &pl) {
    if (!p->acts) return set_error(RNNT_STATUS_INVALID_VALUE, "acts is null");
    if (pl.S_max > 0 && !p->labels) return set_error(RNNT_STATUS_INVALID_VALUE, "labels is null");
    for (int b = 0; b < pl.B; ++b) {
        const int *lab = utt_labels(p, b);
        for (int s = 0; s < p->S_host[b]; ++s)
            if (lab[s] < 0 || lab[s] >= pl.V)
                return set_error(RNNT_STATUS_INVALID_VALUE, "label " + std::to_string(lab[s]) + " at (" +
                                                                std::to_string(b) + ", " + std::to_string(s) +
                                                                ") outside [0, V = " + std::to_string(pl.V) + ")");
    }
    return RNNT_STATUS_SUCCESS;
}

// Workspace views.
struct Views {
    float *den;
    double *lpb, *lpe, *alpha, *beta, *ll, *llb;
    int *min_s, *max_s;
};

Views views(const CpuPlan &pl, void *ws) {
    char *w = static_cast<char *>(ws);
    Views v;
    v.den = reinterpret_cast<float *>(w + pl.off_den);
    v.lpb = reinterpret_cast<double *>(w + pl.off_lpb);
    v.lpe = reinterpret_cast<double *>(w + pl.off_lpe);
    v.alpha = reinterpret_cast<double *>(w + pl.off_alpha);
    v.beta = reinterpret_cast<double *>(w + pl.off_beta);
    v.ll = reinterpret_cast<double *>(w + pl.off_ll);
    v.llb = reinterpret_cast<double *>(w + pl.off_llb);
    v.min_s = pl.align ? reinterpret_cast<int *>(w + pl.off_min) : nullptr;
    v.max_s = pl.align ? reinterpret_cast<int *>(w + pl.off_max) : nullptr;
    return v;
}

// utterance of lattice column c (col_off is increasing)
inline int col_utt(const CpuPlan &pl, int64_t c) {
    return (int)(std::upper_bound(pl.col_off.begin(), pl.col_off.end(), c) - pl.col_off.begin()) - 1;
}

// first acts / grads row of column (b, t) (W = S_b + 1): packed = the lattice row, padded = (b * pad_T + t) * pad_S1
inline int64_t acts_row(const CpuPlan &pl, int b, int t, int W) {
    return pl.pad_S1 ? ((int64_t)b * pl.pad_T + t) * pl.pad_S1 : pl.row_off[b] + (int64_t)t * W;
}

int threads_of(int num_threads) { return num_threads > 0 ? num_threads : omp_get_max_threads(); }

// Padding rows of the padded layout (t >= T_b, or s > S_b) of `out` ([B, pad_T, pad_S1, width], may be null): 0, as
// the HIP path's pad-zero kernel. No-op for the packed layout.
void zero_padding_rows(const mrnnt_problem *p, const CpuPlan &pl, float *out, int64_t width, int nt) {
    if (!pl.pad_S1 || !out) return;
#pragma omp parallel for schedule(static) num_threads(nt)
    for (int64_t pc = 0; pc < (int64_t)pl.B * pl.pad_T; ++pc) {
        const int b = (int)(pc / pl.pad_T), t = (int)(pc % pl.pad_T);
        const int64_t s0 = t < p->T_host[b] ? p->S_host[b] + 1 : 0;
        std::fill(out + (pc * pl.pad_S1 + s0) * width, out + (pc + 1) * pl.pad_S1 * width, 0.0f);
    }
}

// Alignment band (restrict_to_alignment, cpu_workspace_manager.h:207-224): with m(t) = aligned labels among
// the first t frames, alpha(t, .) lives in [m(t+1-k), m(t+1+k)] (indices clamped to [0, T]).
void band_utt(const int *al, int T, int k, int align_blank, int *min_s, int *max_s) {
    std::vector<int> m(T + 1, 0);
    for (int t = 0; t < T; ++t) m[t + 1] = m[t] + (al[t] != align_blank ? 1 : 0);
    for (int t = 0; t < T; ++t) {
        min_s[t] = m[std::min(std::max(0, t + 1 - k), T)];
        max_s[t] = m[std::max(0, std::min(T, t + 1 + k))];
    }
}

void build_band(const mrnnt_problem *p, const CpuPlan &pl, const Views &w, int nt) {
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt)
    for (int b = 0; b < pl.B; ++b) {
        const int64_t c0 = pl.col_off[b];
        band_utt(p->alignment + (int64_t)b * p->align_stride, p->T_host[b], p->max_shift, p->align_blank,
                 w.min_s + c0, w.max_s + c0);
    }
}

// Rows of column (b, t) the recursion can touch: the band max(0, t-(T-S)) <= s <= min(t, S), narrowed under an
// alignment to the rows alpha(t, [min_s(t), max_s(t)]) and beta(t, [min_s(t-1), max_s(t-1)]) read (the HIP
// path's align_window, mrnnt_device.h). Every other row only meets -inf state.
inline void row_window(const Views &w, int64_t c, int t, int T, int S, int &lo, int &hi) {
    lo = std::max(0, t - (T - S));
    hi = std::min(t, S);
    if (!w.min_s) return;
    int wlo = w.min_s[c] - 1, whi = w.max_s[c];
    if (t > 0) {
        wlo = std::min(wlo, w.min_s[c - 1]);
        whi = std::max(whi, w.max_s[c - 1]);
    } else {
        wlo = std::min(wlo, 0);
        whi = std::max(whi, 0);
    }
    lo = std::max(lo, wlo);
    hi = std::min(hi, whi);
}

// log sigmoid(z) = min(z, 0) - log1p(exp(-|z|)): -inf -> -inf, +inf -> 0, NaN -> NaN
inline double log_sigmoid(double z) { return std::fmin(z, 0.0) - std::log1p(std::exp(-std::fabs(z))); }

// The factorised-blank row (mrnnt_cpu_hat_*; the HIP path's HAT bodies and hat_lp, mrnnt_lsm.h): blank a Bernoulli on
// its own logit, the labels a softmax over the other V - 1 logits -- den' = -LSE_{v != blank} from one reduce of the
// row that skips z_blank (it never enters a max or a sum),
//   lpb = log sigmoid(z_b),   lpe = log sigmoid(-z_b) + z_l + den'   (a label equal to blank: no such arc).
// A NaN or +inf logit anywhere in the row makes both NaN (z_b = +inf included), as the standard row. A masked (-inf)
// label logit, and a row whose non-blank logits are all masked (den' = +inf), have no label arc: lpe = -inf.
void hat_row(const float *z, int V, int blank, int label, float *den_out, double *lpb, double *lpe) {
    float m;
    double sum;
    row_max_sum_skip(z, V, blank, m, sum);
    const double den = -(double)m - std::log(sum);
    const double zb = z[blank];
    const bool bad = zb == std::numeric_limits<double>::infinity() || den != den;
    const double ze = label < 0 ? 0.0 : (label == blank ? kNegInf : (double)z[label]);
    constexpr double nan = std::numeric_limits<double>::quiet_NaN();
    *den_out = (float)den;
    *lpb = bad ? nan : log_sigmoid(zb);
    const bool none = ze == kNegInf || den == -kNegInf;
    *lpe = bad ? nan : (none ? kNegInf : log_sigmoid(-zb) + (ze + den));
}

void softmax_pass(const mrnnt_problem *p, const CpuPlan &pl, const Views &w, int nt, bool hat = false) {
    const float *acts = static_cast<const float *>(p->acts);
    const int V = pl.V;
#pragma omp parallel for schedule(dynamic, 4) num_threads(nt)
    for (int64_t c = 0; c < pl.cols; ++c) {
        const int b = col_utt(pl, c);
        const int t = (int)(c - pl.col_off[b]);
        const int T = p->T_host[b], S = p->S_host[b], W = S + 1;
        const int *lab = utt_labels(p, b);
        const int64_t r0 = pl.row_off[b] + (int64_t)t * W;  // lattice row of (t, 0)
        const int64_t a0 = acts_row(pl, b, t, W);           // acts row of (t, 0)
        int lo, hi;
        row_window(w, c, t, T, S, lo, hi);
        for (int s = 0; s < W; ++s) {
            const int64_t r = r0 + s;
            if (s < lo || s > hi) {  // finite filler: the recursion only adds it to -inf state
                w.den[r] = 0.0f;
                w.lpb[r] = 0.0;
                w.lpe[r] = 0.0;
                continue;
            }
            const float *z = acts + (a0 + s) * V;
            if (hat) {
                hat_row(z, V, p->blank, s < S ? lab[s] : -1, &w.den[r], &w.lpb[r], &w.lpe[r]);
                continue;
            }
            float m;
            double sum;
            row_max_sum(z, V, m, sum);
            const double den = -(double)m - std::log(sum);
            w.den[r] = (float)den;
            w.lpb[r] = (double)z[p->blank] + den;
            w.lpe[r] = (s < S) ? (double)z[lab[s]] + den : 0.0;
        }
    }
}

// band(u): the states before frame u, 0 <= u <= T (the bounds of alpha_utt / beta_utt)
inline void state_band(const Views &w, int64_t c0, int T, int S, int u, int &lo, int &hi) {
    lo = std::max(u - (T - S), 0);
    hi = std::min(u, S);
    if (w.min_s && u > 0) {
        lo = std::max(lo, w.min_s[c0 + u - 1]);
        hi = std::min(hi, w.max_s[c0 + u - 1]);
    }
    if (u == 0) hi = 0;
}

// alpha(t, s) = lse(alpha(t-1, s) + lpb(t, s), alpha(t-1, s-1) + lpe(t, s-1)) on
// max(min_s(t), t-(T-1-S)) <= s <= min(max_s(t), t+1), -inf elsewhere (cpu_rnnt.h:140-161,
// cpu_workspace_manager.h:62-64,160-181); returns alpha(T-1, S).
double alpha_utt(const CpuPlan &pl, const Views &w, int b, int T, int S) {
    const int W = S + 1;
    const int64_t r0 = pl.row_off[b], c0 = pl.col_off[b];
    double *A = w.alpha + r0;
    for (int t = 0; t < T; ++t) {
        int lo, hi;
        state_band(w, c0, T, S, t + 1, lo, hi);
        double *a = A + (int64_t)t * W;
        const double *ap = A + (int64_t)(t - 1) * W;
        const double *pb = w.lpb + r0 + (int64_t)t * W;
        const double *pe = w.lpe + r0 + (int64_t)t * W;
        for (int s = 0; s < W; ++s) {
            if (s < lo || s > hi) {
                a[s] = kNegInf;
                continue;
            }
            const double stay = (t == 0) ? (s == 0 ? 0.0 : kNegInf) : ap[s];
            const double move = (s == 0) ? kNegInf : ((t == 0) ? (s == 1 ? 0.0 : kNegInf) : ap[s - 1]);
            a[s] = lse(stay + pb[s], (s == 0) ? kNegInf : move + pe[s - 1]);
        }
    }
    return A[(int64_t)(T - 1) * W + S];
}

// beta(t, s) = lse(beta(t+1, s) + lpb(t, s), beta(t+1, s+1) + lpe(t, s)) on
// max(min_s(t-1), t-(T-S)) <= s <= min(max_s(t-1), t) (t > 0; beta(0, .) is s = 0 only), -inf elsewhere,
// beta(T, s) = [s == S] (cpu_rnnt.h:163-214, cpu_workspace_manager.h:66-85,183-205); returns beta(0, 0).
double beta_utt(const CpuPlan &pl, const Views &w, int b, int T, int S) {
    const int W = S + 1;
    const int64_t r0 = pl.row_off[b], c0 = pl.col_off[b];
    double *Bt = w.beta + r0;
    for (int t = T - 1; t >= 0; --t) {
        int lo, hi;
        state_band(w, c0, T, S, t, lo, hi);
        double *bt = Bt + (int64_t)t * W;
        const double *bn = Bt + (int64_t)(t + 1) * W;
        const double *pb = w.lpb + r0 + (int64_t)t * W;
        const double *pe = w.lpe + r0 + (int64_t)t * W;
        for (int s = 0; s < W; ++s) {
            if (s < lo || s > hi) {
                bt[s] = kNegInf;
                continue;
            }
            const double stay = (t == T - 1) ? (s == S ? 0.0 : kNegInf) : bn[s];
            double move = kNegInf;
            if (s < S) move = ((t == T - 1) ? (s + 1 == S ? 0.0 : kNegInf) : bn[s + 1]) + pe[s];
            bt[s] = lse(stay + pb[s], move);
        }
    }
    return Bt[0];
}

// Best path of one utterance (mrnnt_cpu_align; the HIP path's mrnnt_viterbi.hip): the max-plus recursion
//   v(t, s) = max(v(t-1, s) + lpb(t, s), v(t-1, s-1) + lpe(t, s-1)) on alpha's band, fp64, two rolling rows,
// the label arc taken only when strictly greater than the blank arc (a NaN arc makes the cell NaN), one back-pointer
// byte per cell in the workspace's beta array (unused by this call), then the backtrace from (T-1, S).
// Writes row[0, out_stride): labels / blank for t < T, blank for t >= T; all -1 when v(T-1, S) is not finite.
double viterbi_utt(const mrnnt_problem *p, const CpuPlan &pl, const Views &w, int b, int *row, int64_t out_stride) {
    const int T = p->T_host[b], S = p->S_host[b], W = S + 1;
    const int64_t r0 = pl.row_off[b], c0 = pl.col_off[b];
    unsigned char *bp = reinterpret_cast<unsigned char *>(w.beta + r0);  // [T, W]
    std::vector<double> va(W, kNegInf), vb(W, kNegInf);
    double *prev = va.data(), *cur = vb.data();
    prev[0] = 0.0;  // v(-1, s)
    for (int t = 0; t < T; ++t) {
        int lo, hi;
        state_band(w, c0, T, S, t + 1, lo, hi);
        const double *pb = w.lpb + r0 + (int64_t)t * W;
        const double *pe = w.lpe + r0 + (int64_t)t * W;
        unsigned char *bt = bp + (int64_t)t * W;
        for (int s = 0; s < W; ++s) {
            if (s < lo || s > hi) {
                cur[s] = kNegInf;
                bt[s] = 0;
                continue;
            }
            const double x = prev[s] + pb[s];
            const double y = (s == 0) ? kNegInf : prev[s - 1] + pe[s - 1];
            const bool take = y > x || y != y;
            cur[s] = take ? y : x;
            bt[s] = take ? 1 : 0;
        }
        std::swap(prev, cur);
    }
    const double fin = prev[S];
    if (!std::isfinite(fin)) {
        std::fill(row, row + out_stride, -1);
        return fin;
    }
    const int *lab = utt_labels(p, b);
    int s = S;
    for (int t = T - 1; t >= 0; --t) {
        const int bit = (s > 0 && bp[(int64_t)t * W + s]) ? 1 : 0;
        row[t] = bit ? lab[s - 1] : p->blank;
        s -= bit;
    }
    std::fill(row + T, row + out_stride, p->blank);
    return fin;
}

// The label of slot s where row (t, s) has a label arc, else -1: s = S, a label outside [0, V), and a label equal to
// blank (no such arc) have none.
inline int slot_label(const int *lab, int s, int S, int V, int blank) {
    return (s < S && (unsigned)lab[s] < (unsigned)V && lab[s] != blank) ? lab[s] : -1;
}

// Column (b, t) of one utterance: its monotonic band [lo, hi], ll, and the recursion state around the two arcs that
// leave node (t, s), with the lattice's edge rules in one place: before the first frame alpha is [s == 0], after the
// last one beta is [s == S] (so [s + 1 == S] behind the label arc), and row s = S has no label arc. Every read stays
// inside the utterance's own T (S + 1) rows.
struct ArcState {
    const double *A, *Bt;  // alpha / beta of the utterance, [T, W]
    int t, T, S, W, lo, hi;
    double ll;
    ArcState(const CpuPlan &pl, const Views &w, int b, int t_, int T_, int S_)
        : A(w.alpha + pl.row_off[b]), Bt(w.beta + pl.row_off[b]), t(t_), T(T_), S(S_), W(S_ + 1),
          lo(std::max(0, t_ - (T_ - S_))), hi(std::min(t_, S_)), ll(w.ll[b]) {}
    bool in_band(int s) const { return s >= lo && s <= hi; }
    // alpha(t-1, s)
    double alpha_in(int s) const { return (t == 0) ? (s == 0 ? 0.0 : kNegInf) : A[(int64_t)(t - 1) * W + s]; }
    // beta(t, s)
    double beta_at(int s) const { return Bt[(int64_t)t * W + s]; }
    // beta(t+1, s): behind the blank arc
    double beta_blank(int s) const { return (t == T - 1) ? (s == S ? 0.0 : kNegInf) : Bt[(int64_t)(t + 1) * W + s]; }
    // beta(t+1, s+1): behind the label arc
    double beta_label(int s) const {
        return (s == S) ? kNegInf : ((t == T - 1) ? (s + 1 == S ? 0.0 : kNegInf) : Bt[(int64_t)(t + 1) * W + s + 1]);
    }
};

// ---- the dense-gradient pass over row policies (the HIP path's grad_staged_kernel<..., P>, mrnnt_grad.h) -------------
//
// grad_pass walks every lattice column (b, t), OpenMP over columns, and every row s in [0, S] of it: the row is either
// filled with one value without reading acts, or written by the policy's row formula; then the padding rows of the
// padded layout are zeroed. A row policy P (named after its HIP twin) supplies exactly what differs:
//   P::Col column(c, b, t, T, S)         what a column sets up once
//   bool row(col, s, r, a, fill, live)   row s (lattice row r, acts row a): its coefficients, then either false and the
//                                        value a dead or out-of-band row is filled with, or the row formula on live()
struct RowsBase {
    const mrnnt_problem *p;
    const CpuPlan &pl;
    const Views &w;
};

// a live row as grad_pass hands it to the row formula: g[0, V) from z[0, V) (g may be z itself)
struct RowIO {
    const float *z;
    float *g;
    int l;         // slot_label
    float zb, zl;  // z[blank], z[l] (0 without a label arc)
};

template <class P>
void grad_pass(const P &rows, float *grads, int nt) {
    const mrnnt_problem *p = rows.p;
    const CpuPlan &pl = rows.pl;
    const float *acts = static_cast<const float *>(p->acts);
    const int V = pl.V, blank = p->blank;
#pragma omp parallel for schedule(dynamic, 4) num_threads(nt)
    for (int64_t c = 0; c < pl.cols; ++c) {
        const int b = col_utt(pl, c);
        const int t = (int)(c - pl.col_off[b]);
        const int T = p->T_host[b], S = p->S_host[b], W = S + 1;
        const int *lab = utt_labels(p, b);
        const int64_t r0 = pl.row_off[b] + (int64_t)t * W, a0 = acts_row(pl, b, t, W);
        const typename P::Col col = rows.column(c, b, t, T, S);
        for (int s = 0; s < W; ++s) {
            float *g = grads + (a0 + s) * V;
            const auto live = [&] {
                const float *z = acts + (a0 + s) * V;
                const int l = slot_label(lab, s, S, V, blank);
                return RowIO{z, g, l, z[blank], l >= 0 ? z[l] : 0.0f};  // read first: grads may alias acts
            };
            float fill;
            if (!rows.row(col, s, r0 + s, a0 + s, fill, live)) std::fill(g, g + V, fill);  // acts not read
        }
    }
    zero_padding_rows(p, pl, grads, V, nt);
}

// The loss gradient (mrnnt_cpu_backward; cpu_rnnt.h:216-249):
//   g[v] = e^(z[v] + den + alpha(t-1,s) + beta(t,s) - ll) - [v == blank] e^(lpb + alpha(t-1,s) + beta(t+1,s) - ll)
//          - [v == label(s), label != blank] e^(lpe + alpha(t-1,s) + beta(t+1,s+1) - ll),
// times grad_scale[b]. Out-of-band rows are 0 * scale (NaN * scale for ll = -inf: the reference's exp(... - ll)),
// in-band rows below the occupancy threshold (kDeadLogOcc) are exact zeros written without reading acts, and so are
// the rows whose every vexp flushes to 0 (kFlushLnCpu).
struct LossRows : RowsBase {
    const float *scale;
    struct Col : ArcState {
        float sc, zero;
    };
    Col column(int64_t, int b, int t, int T, int S) const {
        const ArcState band(pl, w, b, t, T, S);
        const float sc = scale ? scale[p->grad_scale_broadcast ? 0 : b] : 1.0f;
        return {band, sc, (band.ll > kNegInf ? 0.0f : std::numeric_limits<float>::quiet_NaN()) * sc};
    }
    template <class Live>
    bool row(const Col &col, int s, int64_t r, int64_t, float &fill, Live &&live) const {
        fill = col.zero;
        if (!col.in_band(s)) return false;
        const double b0 = col.beta_at(s), base = col.alpha_in(s) - col.ll;
        fill = 0.0f * col.sc;
        if (base + b0 < mrnnt::kDeadLogOcc) return false;
        const float den = w.den[r];
        const float c = (float)((double)den + base + b0), sc = col.sc;
        const float cb = (float)std::exp(w.lpb[r] + base + col.beta_blank(s));
        // (the label arc's state is read only where the formula below reads it: s < S, whatever the label is)
        const float ce = s < col.S ? (float)std::exp(w.lpe[r] + base + col.beta_label(s)) : 0.0f;
        // flush-dead (mrnnt_host.h kFlushLnCpu): every vexp below is exactly 0 and so are both corrections; the row
        // is (0 - 0) * sc = fill, acts not read. A NaN anywhere compares false and takes the formula.
        if (g_flush_rows && (double)c - (double)den < mrnnt::kFlushLnCpu && cb == 0.0f && ce == 0.0f) return false;
        const RowIO io = live();
        grad_row(io.z, io.g, pl.V, c, sc);
        io.g[p->blank] = (vexp(io.zb + c) - cb) * sc;
        if (io.l >= 0) io.g[io.l] = (vexp(io.zl + c) - ce) * sc;
        return true;
    }
};

// The factorised-blank gradient (mrnnt_cpu_hat_backward; the HIP path's HatRows, mrnnt_hat.hip): with cb / ce the
// blank / label arc posteriors of the row,
//   g[blank] = ce sigmoid(z_b) - cb sigmoid(-z_b),   g[v != blank] = ce (e^(z_v + den') - [v == label(s)]),
// times grad_scale[b], each sigmoid from lpb = log sigmoid(z_b) by itself (sigmoid(-z_b) = -expm1(lpb)). A row whose ce
// and blank element are both zero in fp32 is stored without reading acts, as the out-of-band rows of LossRows are.
struct HatRows : LossRows {
    template <class Live>
    bool row(const Col &col, int s, int64_t r, int64_t, float &fill, Live &&live) const {
        fill = col.zero;
        if (!col.in_band(s)) return false;
        const double base = col.alpha_in(s) - col.ll;
        const double q = w.lpb[r];
        const double le = w.lpe[r] + base + col.beta_label(s);
        const float cb = (float)std::exp(q + base + col.beta_blank(s));
        const float ce = s < col.S ? (float)std::exp(le) : 0.0f;
        // (s = S: no label arc, ce = 0 and its term is absent)
        const float gb = s < col.S ? (float)((double)ce * std::exp(q) - (double)cb * -std::expm1(q))
                                       : (float)((double)cb * std::expm1(q));
        if (ce == 0.0f && gb == 0.0f) return false;
        const RowIO io = live();
        const float sc = col.sc;
        if (ce != 0.0f) {  // (ce = 0: no label arc, every non-blank element is 0 -- s = S, or every label masked)
            const float c = (float)((double)w.den[r] + le);
            grad_row(io.z, io.g, pl.V, c, sc);
            if (io.l >= 0) io.g[io.l] = (vexp(io.zl + c) - ce) * sc;
        } else {
            std::fill(io.g, io.g + pl.V, 0.0f * sc);
        }
        io.g[p->blank] = gb * sc;
        return true;
    }
};

// One row under two signed arc weights, Wb on the blank arc and We on the label arc (mrnnt_cpu_path_backward /
// mrnnt_cpu_expect_backward; the HIP path's WeightRows::grad, mrnnt_grad.h):
//   g[v] = (Wb + We) e^(z_v + den) - [v == blank] Wb - [v == label] We.
inline void weight_row(const RowIO &io, int V, int blank, float den, double, double Wb, double We) {
    grad_row(io.z, io.g, V, den, (float)(Wb + We));
    io.g[blank] -= (float)Wb;
    if (io.l >= 0) io.g[io.l] -= (float)We;
}

// The same for a factorised-blank row (mrnnt_cpu_hat_path_backward / mrnnt_cpu_hat_expect_backward; the HIP path's
// HatWeightRows, mrnnt_grad.h), in fp64 with the library exp / expm1:
//   g[blank] = We sigmoid(z_b) - Wb sigmoid(-z_b),   g[v != blank] = We (e^(z_v + den') - [v == label]),
// sigmoid(z_b) = e^lpb and sigmoid(-z_b) = -expm1(lpb), each by itself. den' = +inf (every label masked): no label arc,
// the non-blank elements are exact zeros. A NaN lpb (z_b NaN or +inf) makes the whole row NaN.
inline void hat_weight_row(const RowIO &io, int V, int blank, float den, double lpb, double Wb, double We) {
    const float gb = (float)(We * std::exp(lpb) - Wb * -std::expm1(lpb));
    if (den == std::numeric_limits<float>::infinity() && lpb == lpb) {
        std::fill(io.g, io.g + V, 0.0f);
    } else {
        const double d = lpb == lpb ? (double)den : lpb;
        for (int v = 0; v < V; ++v)
            io.g[v] = (float)(We * (std::exp((double)io.z[v] + d) - (v == io.l ? 1.0 : 0.0)));
    }
    io.g[blank] = gb;
}

// A weight policy P (column; weights: the two arc weights of a row, false: both zero) under the row formula F
template <class P, auto F>
struct WeightedRows : P {
    template <class Live>
    bool row(const typename P::Col &col, int s, int64_t r, int64_t a, float &fill, Live &&live) const {
        double Wb, We;
        if (!this->weights(col, s, r, a, Wb, We, fill)) return false;
        F(live(), this->pl.V, this->p->blank, this->w.den[r], this->w.lpb[r], Wb, We);
        return true;
    }
};

// Arc posteriors of row (t, s) inside the monotonic band (mrnnt_cpu_posteriors; the HIP path's row_post,
// mrnnt_posterior.hip): the blank and label corrections of LossRows in fp64,
//   bp = e^(lpb + alpha(t-1,s) + beta(t+1,s) - ll),  ep = e^(lpe + alpha(t-1,s) + beta(t+1,s+1) - ll)  (0 at s = S).
// An unreachable row (alpha(t-1,s) or beta(t,s) = -inf) is exactly 0, decided before lp is read.
inline void row_posteriors(const CpuPlan &pl, const Views &w, int b, const ArcState &col, int s, double *bp, double *ep) {
    *bp = *ep = 0.0;
    const double am = col.alpha_in(s);
    if (am == kNegInf || col.beta_at(s) == kNegInf) return;
    const int64_t r = pl.row_off[b] + (int64_t)col.t * col.W + s;
    const double base = am - col.ll;
    *bp = std::exp(w.lpb[r] + base + col.beta_blank(s));
    if (s < col.S) *ep = std::exp(w.lpe[r] + base + col.beta_label(s));
}

}  // namespace

// =================================================================================================
// flat C entry points

extern "C" {

RNNTStatus mrnnt_cpu_workspace_size(const mrnnt_problem *p, size_t *bytes) {
    return plan_bytes<CpuPlan>(bytes, [&](CpuPlan *pl) { return make_cpu_plan(p, pl); });
}

static RNNTStatus cpu_forward_impl(const mrnnt_problem *p, void *ws, size_t ws_bytes, float *costs, int with_beta,
                                   int num_threads, bool hat) {
    CpuPlan pl;
    RNNTStatus st = make_cpu_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_inputs(p, pl)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_workspace(ws, ws_bytes, pl.total)) != RNNT_STATUS_SUCCESS) return st;
    const Views w = views(pl, ws);
    const int nt = threads_of(num_threads);
    if (pl.align) build_band(p, pl, w, nt);
    softmax_pass(p, pl, w, nt, hat);
    const int dirs = with_beta ? 2 : 1;
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt)
    for (int i = 0; i < pl.B * dirs; ++i) {
        const int b = i / dirs;
        const int T = p->T_host[b], S = p->S_host[b];
        if (i % dirs == 0) {
            const double ll = alpha_utt(pl, w, b, T, S);
            w.ll[b] = ll;
            if (costs) costs[b] = (float)(-ll);
        } else {
            w.llb[b] = beta_utt(pl, w, b, T, S);
        }
    }
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_cpu_forward(const mrnnt_problem *p, void *ws, size_t ws_bytes, float *costs, int with_beta,
                             int num_threads) {
    return cpu_forward_impl(p, ws, ws_bytes, costs, with_beta, num_threads, false);
}

RNNTStatus mrnnt_cpu_hat_forward(const mrnnt_problem *p, void *ws, size_t ws_bytes, float *costs, int with_beta,
                                 int num_threads) {
    return cpu_forward_impl(p, ws, ws_bytes, costs, with_beta, num_threads, true);
}

static RNNTStatus cpu_align_impl(const mrnnt_problem *p, void *ws, size_t ws_bytes, int *alignment_out,
                                 int64_t out_stride, float *costs, int num_threads, bool hat) {
    CpuPlan pl;
    RNNTStatus st = make_cpu_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (!alignment_out) return set_error(RNNT_STATUS_INVALID_VALUE, "alignment_out is null");
    if (out_stride < pl.T_max)
        return set_error(RNNT_STATUS_INVALID_VALUE, "alignment_out row stride " + std::to_string(out_stride) +
                                                        " < max input length " + std::to_string(pl.T_max));
    if ((st = check_inputs(p, pl)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_workspace(ws, ws_bytes, pl.total)) != RNNT_STATUS_SUCCESS) return st;
    const Views w = views(pl, ws);
    const int nt = threads_of(num_threads);
    // p->alignment may be alignment_out itself: the band is built from it before any row is written
    if (pl.align) build_band(p, pl, w, nt);
    softmax_pass(p, pl, w, nt, hat);
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt)
    for (int b = 0; b < pl.B; ++b) {
        const double fin = viterbi_utt(p, pl, w, b, alignment_out + (int64_t)b * out_stride, out_stride);
        if (costs) costs[b] = (float)(-fin);
    }
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_cpu_align(const mrnnt_problem *p, void *ws, size_t ws_bytes, int *alignment_out, int64_t out_stride,
                           float *costs, int num_threads) {
    return cpu_align_impl(p, ws, ws_bytes, alignment_out, out_stride, costs, num_threads, false);
}

RNNTStatus mrnnt_cpu_hat_align(const mrnnt_problem *p, void *ws, size_t ws_bytes, int *alignment_out,
                               int64_t out_stride, float *costs, int num_threads) {
    return cpu_align_impl(p, ws, ws_bytes, alignment_out, out_stride, costs, num_threads, true);
}

static RNNTStatus cpu_backward_impl(const mrnnt_problem *p, const void *ws, const float *grad_scale, float *grads,
                                    int num_threads, bool hat) {
    CpuPlan pl;
    RNNTStatus st = make_cpu_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (!p->acts) return set_error(RNNT_STATUS_INVALID_VALUE, "acts is null");
    if (!ws) return set_error(RNNT_STATUS_INVALID_VALUE, "workspace is null");
    if (!grads) return set_error(RNNT_STATUS_INVALID_VALUE, "grads is null");
    const Views w = views(pl, const_cast<void *>(ws));
    const int nt = threads_of(num_threads);
    if (hat) grad_pass(HatRows{{{p, pl, w}, grad_scale}}, grads, nt);
    else grad_pass(LossRows{{p, pl, w}, grad_scale}, grads, nt);
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_cpu_backward(const mrnnt_problem *p, const void *ws, const float *grad_scale, float *grads,
                              int num_threads) {
    return cpu_backward_impl(p, ws, grad_scale, grads, num_threads, false);
}

RNNTStatus mrnnt_cpu_hat_backward(const mrnnt_problem *p, const void *ws, const float *grad_scale, float *grads,
                                  int num_threads) {
    return cpu_backward_impl(p, ws, grad_scale, grads, num_threads, true);
}

#ifdef MRNNT_DEVTOOLS
// development build only: the flush-dead rule of mrnnt_cpu_backward on (1) / off (0); < 0 asks; returns the previous
__attribute__((visibility("default"))) int mrnnt_cpu_flush_rows(int on) {
    const int prev = g_flush_rows;
    if (on >= 0) g_flush_rows = on != 0;
    return prev;
}
#endif

RNNTStatus mrnnt_cpu_posteriors(const mrnnt_problem *p, const void *ws, float *blank_post, float *label_post, float *emit,
                                int64_t emit_stride, float *label_time, int64_t time_stride, int num_threads) {
    CpuPlan pl;
    RNNTStatus st = make_cpu_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (emit && emit_stride < pl.T_max)
        return set_error(RNNT_STATUS_INVALID_VALUE, "emit row stride " + std::to_string(emit_stride) +
                                                        " < max input length " + std::to_string(pl.T_max));
    if (label_time && time_stride < pl.S_max)
        return set_error(RNNT_STATUS_INVALID_VALUE, "label_time row stride " + std::to_string(time_stride) +
                                                        " < max label length " + std::to_string(pl.S_max));
    if (!ws) return set_error(RNNT_STATUS_INVALID_VALUE, "workspace is null");
    const Views w = views(pl, const_cast<void *>(ws));
    const int nt = threads_of(num_threads);
    constexpr float nan = std::numeric_limits<float>::quiet_NaN();
    if (blank_post || label_post || emit) {
#pragma omp parallel for schedule(dynamic, 16) num_threads(nt)
        for (int64_t c = 0; c < pl.cols; ++c) {
            const int b = col_utt(pl, c);
            const int t = (int)(c - pl.col_off[b]);
            const int T = p->T_host[b], S = p->S_host[b], W = S + 1;
            const ArcState col(pl, w, b, t, T, S);
            const bool fin = std::isfinite(col.ll);
            const int64_t a0 = acts_row(pl, b, t, W);
            double sum = 0.0;
            for (int s = 0; s < W; ++s) {
                double bp = 0.0, ep = 0.0;
                if (fin && col.in_band(s)) row_posteriors(pl, w, b, col, s, &bp, &ep);
                if (blank_post) blank_post[a0 + s] = fin ? (float)bp : nan;
                if (label_post) label_post[a0 + s] = fin ? (float)ep : nan;
                sum += ep;
            }
            if (emit) emit[(int64_t)b * emit_stride + t] = fin ? (float)sum : nan;
        }
    }
    if (emit)
        for (int b = 0; b < pl.B; ++b)
            std::fill(emit + (int64_t)b * emit_stride + p->T_host[b], emit + (int64_t)(b + 1) * emit_stride, 0.0f);
    for (float *out : {blank_post, label_post}) zero_padding_rows(p, pl, out, 1, nt);
    if (label_time) {
        std::vector<int64_t> lab_off(pl.B + 1, 0);  // (utterance, label) pairs, one sum along t each
        for (int b = 0; b < pl.B; ++b) lab_off[b + 1] = lab_off[b] + p->S_host[b];
#pragma omp parallel for schedule(dynamic, 8) num_threads(nt)
        for (int64_t i = 0; i < lab_off[pl.B]; ++i) {
            const int b = (int)(std::upper_bound(lab_off.begin(), lab_off.end(), i) - lab_off.begin()) - 1;
            const int s = (int)(i - lab_off[b]);
            const int T = p->T_host[b], S = p->S_host[b];
            double sum = 0.0;
            for (int t = s; t <= s + (T - S); ++t) {  // the frames with (t, s) inside the band
                double bp, ep;
                row_posteriors(pl, w, b, ArcState(pl, w, b, t, T, S), s, &bp, &ep);
                sum += (double)t * ep;
            }
            label_time[(int64_t)b * time_stride + s] = std::isfinite(w.ll[b]) ? (float)sum : nan;
        }
        for (int b = 0; b < pl.B; ++b)
            std::fill(label_time + (int64_t)b * time_stride + p->S_host[b], label_time + (int64_t)(b + 1) * time_stride,
                      -1.0f);
    }
    return RNNT_STATUS_SUCCESS;
}

// mrnnt_sample on the host (the HIP path's mrnnt_sample.hip): the same walk with the random numbers and the decision
// rule of mrnnt_sample.h, one (utterance, sample) per loop iteration.
RNNTStatus mrnnt_cpu_sample(const mrnnt_problem *p, const void *ws, int num_samples, uint64_t seed, int64_t first_sample,
                            int *alignments, int64_t out_stride, float *path_costs, int num_threads) {
    CpuPlan pl;
    RNNTStatus st = make_cpu_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (num_samples < 1)
        return set_error(RNNT_STATUS_INVALID_VALUE, "num_samples must be >= 1, got " + std::to_string(num_samples));
    if (first_sample < 0 || first_sample + (int64_t)num_samples > ((int64_t)1 << 32))
        return set_error(RNNT_STATUS_INVALID_VALUE, "sample indices [first_sample, first_sample + num_samples) = [" +
                                                        std::to_string(first_sample) + ", " +
                                                        std::to_string(first_sample + (int64_t)num_samples) +
                                                        ") must lie in [0, 2^32]");
    if (!alignments) return set_error(RNNT_STATUS_INVALID_VALUE, "alignments is null");
    if (out_stride < pl.T_max)
        return set_error(RNNT_STATUS_INVALID_VALUE, "alignments row stride " + std::to_string(out_stride) +
                                                        " < max input length " + std::to_string(pl.T_max));
    if (!ws) return set_error(RNNT_STATUS_INVALID_VALUE, "workspace is null");
    if (pl.S_max > 0 && !p->labels) return set_error(RNNT_STATUS_INVALID_VALUE, "labels is null");
    const Views w = views(pl, const_cast<void *>(ws));
    const int nt = threads_of(num_threads);
    constexpr float nan = std::numeric_limits<float>::quiet_NaN();
#pragma omp parallel for schedule(dynamic, 8) num_threads(nt)
    for (int64_t i = 0; i < (int64_t)pl.B * num_samples; ++i) {
        const int b = (int)(i / num_samples);
        const int T = p->T_host[b], S = p->S_host[b], W = S + 1;
        int *row = alignments + i * out_stride;
        const double ll = w.ll[b];
        if (!std::isfinite(ll)) {  // -inf: no path (+inf cost); NaN / +inf: NaN
            std::fill(row, row + out_stride, -1);
            if (path_costs) path_costs[i] = ll == kNegInf ? std::numeric_limits<float>::infinity() : nan;
            continue;
        }
        const int *lab = utt_labels(p, b);
        const uint32_t smp = (uint32_t)(first_sample + i % num_samples);
        const double *pb = w.lpb + pl.row_off[b], *pe = w.lpe + pl.row_off[b];
        uint32_t word[4] = {0, 0, 0, 0};
        int s = 0;
        double cost = 0.0;
        for (int t = 0; t < T; ++t) {
            if ((t & 3) == 0) mrnnt::sample_block(seed, (uint32_t)(t >> 2), smp, (uint32_t)b, word);
            const int64_t r = (int64_t)t * W + s;
            const ArcState arc(pl, w, b, t, T, S);
            double x = kNegInf, y = kNegInf;
            if (T - 1 - t >= S - s) x = pb[r] + arc.beta_blank(s);  // else the blank arc leaves the band
            if (s < S) y = pe[r] + arc.beta_label(s);
            const bool take = mrnnt::sample_uniform(word[t & 3]) < mrnnt::sample_p_label(x, y) && s < S;
            cost += take ? pe[r] : pb[r];
            row[t] = take ? lab[s] : p->blank;
            s += take ? 1 : 0;
        }
        std::fill(row + T, row + out_stride, p->blank);
        if (path_costs) path_costs[i] = (float)(-cost);
    }
    return RNNT_STATUS_SUCCESS;
}

}  // extern "C"

// ---- mrnnt_cpu_path_*: scores of given alignments and their logit gradient (the HIP path's mrnnt_path.hip) ----------
namespace {

constexpr int kHullEmpty = 1 << 29;

struct CpuPathPlan {
    CpuPlan pl;
    size_t off_valid = 0, total = 0;
};

// the plan (with band arrays: the hull) and the host checks, in the order of the HIP path's
RNNTStatus make_cpu_path_plan(const mrnnt_problem *p, int num_paths, const int *alignments, int64_t path_stride,
                              bool sizing, CpuPathPlan *pp) {
    if (p && p->alignment)
        return set_error(RNNT_STATUS_INVALID_VALUE, "path scores take no restricting alignment (p->alignment must be "
                                                    "NULL: the band arrays hold the hull of the given paths)");
    if (num_paths < 1)
        return set_error(RNNT_STATUS_INVALID_VALUE, "num_paths must be >= 1, got " + std::to_string(num_paths));
    const RNNTStatus st = make_cpu_plan(p, &pp->pl, true);
    if (st != RNNT_STATUS_SUCCESS) return st;
    Carver ws{pp->pl.total};
    pp->off_valid = ws.take(sizeof(int) * (size_t)pp->pl.B * num_paths);
    pp->total = ws.at;
    if (sizing) return RNNT_STATUS_SUCCESS;
    if (!alignments) return set_error(RNNT_STATUS_INVALID_VALUE, "alignments is null");
    if (path_stride < pp->pl.T_max)
        return set_error(RNNT_STATUS_INVALID_VALUE, "alignments row stride " + std::to_string(path_stride) +
                                                        " < max input length " + std::to_string(pp->pl.T_max));
    return RNNT_STATUS_SUCCESS;
}

// The walk of one alignment row: calls visit(t, s, label_arc) for every frame while the row is valid; returns
// validity (every entry blank or labels[b, s] with s < S, and s == S at the end).
template <class F>
inline bool walk_path(const int *row, const int *lab, int T, int S, int blank, F &&visit) {
    int s = 0;
    for (int t = 0; t < T; ++t) {
        const int v = row[t];
        if (v == blank) {
            visit(t, s, false);
        } else if (v >= 0 && s < S && v == lab[s]) {
            visit(t, s, true);
            ++s;
        } else {
            return false;
        }
    }
    return s == S;
}

// The path-score gradient (mrnnt_cpu_path_backward; the HIP path's PathRows / HatPathRows, mrnnt_path.hip): the arc
// weights are the sums the caller left in w.alpha (Wb) / w.beta (We) over the hull rows; a row outside the hull, or
// with both weights zero, is exact zeros.
struct PathWeights : RowsBase {
    struct Col {
        int lo, hi;
    };
    Col column(int64_t c, int, int, int, int S) const { return {w.min_s[c] - 1, std::min(w.max_s[c], S)}; }
    bool weights(const Col &col, int s, int64_t r, int64_t, double &Wb, double &We, float &fill) const {
        const bool in = s >= col.lo && s <= col.hi;
        Wb = in ? w.alpha[r] : 0.0;
        We = in ? w.beta[r] : 0.0;
        fill = 0.0f;
        return Wb != 0.0 || We != 0.0;
    }
};
using PathRows = WeightedRows<PathWeights, weight_row>;
using HatPathRows = WeightedRows<PathWeights, hat_weight_row>;

}  // namespace

extern "C" {

RNNTStatus mrnnt_cpu_path_workspace_size(const mrnnt_problem *p, int num_paths, size_t *bytes) {
    return plan_bytes<CpuPathPlan>(
        bytes, [&](CpuPathPlan *pp) { return make_cpu_path_plan(p, num_paths, nullptr, 0, true, pp); });
}

// mrnnt_cpu_path_forward / mrnnt_cpu_hat_path_forward
static RNNTStatus cpu_path_forward_impl(const mrnnt_problem *p, void *ws, size_t ws_bytes, const int *alignments,
                                        int num_paths, int64_t path_stride, float *path_costs, int num_threads,
                                        bool hat) {
    CpuPathPlan pp;
    RNNTStatus st = make_cpu_path_plan(p, num_paths, alignments, path_stride, false, &pp);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const CpuPlan &pl = pp.pl;
    if ((st = check_inputs(p, pl)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = check_workspace(ws, ws_bytes, pp.total)) != RNNT_STATUS_SUCCESS) return st;
    const Views w = views(pl, ws);
    int *valid = reinterpret_cast<int *>(static_cast<char *>(ws) + pp.off_valid);
    const int nt = threads_of(num_threads);
    const int K = num_paths;
    // validity, and the hull of the valid paths in the band arrays: min_s = lowest visited row + 1, max_s = highest --
    // the form whose alignment window (row_window) is exactly [lowest, highest]; no valid path: no rows
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt)
    for (int b = 0; b < pl.B; ++b) {
        const int T = p->T_host[b], S = p->S_host[b];
        const int *lab = utt_labels(p, b);
        int *lo = w.min_s + pl.col_off[b], *hi = w.max_s + pl.col_off[b];
        std::fill(lo, lo + T, kHullEmpty - 1);
        std::fill(hi, hi + T, -1);
        for (int k = 0; k < K; ++k) {
            const int *row = alignments + ((int64_t)b * K + k) * path_stride;
            const bool ok = walk_path(row, lab, T, S, p->blank, [](int, int, bool) {});
            valid[(int64_t)b * K + k] = ok ? 1 : 0;
            if (ok)
                walk_path(row, lab, T, S, p->blank, [&](int t, int s, bool) {
                    lo[t] = std::min(lo[t], s);
                    hi[t] = std::max(hi[t], s);
                });
        }
        for (int t = 0; t < T; ++t) lo[t] += 1;
    }
    softmax_pass(p, pl, w, nt, hat);
    if (!path_costs) return RNNT_STATUS_SUCCESS;
#pragma omp parallel for schedule(dynamic, 8) num_threads(nt)
    for (int64_t i = 0; i < (int64_t)pl.B * K; ++i) {
        const int b = (int)(i / K);
        if (!valid[i]) {
            path_costs[i] = std::numeric_limits<float>::infinity();
            continue;
        }
        const int T = p->T_host[b], S = p->S_host[b], W = S + 1;
        const int *lab = utt_labels(p, b);
        const double *pb = w.lpb + pl.row_off[b], *pe = w.lpe + pl.row_off[b];
        double sum = 0.0;
        walk_path(alignments + i * path_stride, lab, T, S, p->blank, [&](int t, int s, bool label) {
            const int64_t r = (int64_t)t * W + s;
            sum += label ? pe[r] : pb[r];
        });
        path_costs[i] = (float)(-sum);
    }
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_cpu_path_forward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const int *alignments,
                                  int num_paths, int64_t path_stride, float *path_costs, int num_threads) {
    return cpu_path_forward_impl(p, ws, ws_bytes, alignments, num_paths, path_stride, path_costs, num_threads, false);
}

RNNTStatus mrnnt_cpu_hat_path_forward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const int *alignments,
                                      int num_paths, int64_t path_stride, float *path_costs, int num_threads) {
    return cpu_path_forward_impl(p, ws, ws_bytes, alignments, num_paths, path_stride, path_costs, num_threads, true);
}

// mrnnt_cpu_path_backward / mrnnt_cpu_hat_path_backward
static RNNTStatus cpu_path_backward_impl(const mrnnt_problem *p, void *ws, size_t ws_bytes, const int *alignments,
                                         int num_paths, int64_t path_stride, const float *weights, float *grads,
                                         int num_threads, bool hat) {
    CpuPathPlan pp;
    RNNTStatus st = make_cpu_path_plan(p, num_paths, alignments, path_stride, false, &pp);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const CpuPlan &pl = pp.pl;
    if (!p->acts) return set_error(RNNT_STATUS_INVALID_VALUE, "acts is null");
    if (pl.S_max > 0 && !p->labels) return set_error(RNNT_STATUS_INVALID_VALUE, "labels is null");
    if (!grads) return set_error(RNNT_STATUS_INVALID_VALUE, "grads is null");
    if ((st = check_workspace(ws, ws_bytes, pp.total)) != RNNT_STATUS_SUCCESS) return st;
    const Views w = views(pl, ws);
    const int *valid = reinterpret_cast<const int *>(static_cast<const char *>(ws) + pp.off_valid);
    const int nt = threads_of(num_threads);
    const int K = num_paths;
    // Wb (w.alpha) / We (w.beta): zero over the hull rows, then the valid paths' weights in ascending k
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt)
    for (int b = 0; b < pl.B; ++b) {
        const int T = p->T_host[b], S = p->S_host[b], W = S + 1;
        const int *lab = utt_labels(p, b);
        const int *lo = w.min_s + pl.col_off[b], *hi = w.max_s + pl.col_off[b];
        double *wb = w.alpha + pl.row_off[b], *we = w.beta + pl.row_off[b];
        for (int t = 0; t < T; ++t)
            for (int s = std::max(lo[t] - 1, 0); s <= std::min(hi[t], S); ++s) wb[(int64_t)t * W + s] = we[(int64_t)t * W + s] = 0.0;
        for (int k = 0; k < K; ++k) {
            if (!valid[(int64_t)b * K + k]) continue;
            const double wk = weights ? (double)weights[(int64_t)b * K + k] : 1.0;
            walk_path(alignments + ((int64_t)b * K + k) * path_stride, lab, T, S, p->blank, [&](int t, int s, bool label) {
                if (s < lo[t] - 1 || s > hi[t]) return;  // (a workspace that is not this call's forward's: stay in the hull)
                (label ? we : wb)[(int64_t)t * W + s] += wk;
            });
        }
    }
    if (hat) grad_pass(HatPathRows{{{p, pl, w}}}, grads, nt);
    else grad_pass(PathRows{{{p, pl, w}}}, grads, nt);
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_cpu_path_backward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const int *alignments,
                                   int num_paths, int64_t path_stride, const float *weights, float *grads,
                                   int num_threads) {
    return cpu_path_backward_impl(p, ws, ws_bytes, alignments, num_paths, path_stride, weights, grads, num_threads,
                                  false);
}

RNNTStatus mrnnt_cpu_hat_path_backward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const int *alignments,
                                       int num_paths, int64_t path_stride, const float *weights, float *grads,
                                       int num_threads) {
    return cpu_path_backward_impl(p, ws, ws_bytes, alignments, num_paths, path_stride, weights, grads, num_threads,
                                  true);
}

RNNTStatus mrnnt_cpu_read_state(const mrnnt_problem *p, const void *ws, float *den, double *alpha, double *beta) {
    CpuPlan pl;
    RNNTStatus st = make_cpu_plan(p, &pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (!ws) return set_error(RNNT_STATUS_INVALID_VALUE, "workspace is null");
    const Views w = views(pl, const_cast<void *>(ws));
    if (den) std::memcpy(den, w.den, sizeof(float) * pl.N);
    if (alpha) std::memcpy(alpha, w.alpha, sizeof(double) * pl.N);
    if (beta) std::memcpy(beta, w.beta, sizeof(double) * pl.N);
    return RNNT_STATUS_SUCCESS;
}

}  // extern "C"

// ---- mrnnt_cpu_expect_*: expected path costs and their logit gradient (the HIP path's mrnnt_expect.hip) -------------
namespace {

struct CpuExpectPlan {
    CpuPlan pl;
    size_t off_A = 0, off_Bk = 0, off_R = 0, total = 0;  // the cost states A / Bk [N], the expectations R [B]
    static double *view(void *ws, size_t off) { return reinterpret_cast<double *>(static_cast<char *>(ws) + off); }
};

RNNTStatus make_cpu_expect_plan(const mrnnt_problem *p, CpuExpectPlan *ep) {
    const RNNTStatus st = make_cpu_plan(p, &ep->pl);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const CpuPlan &pl = ep->pl;
    Carver ws{pl.total};
    ep->off_A = ws.take(sizeof(double) * (size_t)pl.N);
    ep->off_Bk = ws.take(sizeof(double) * (size_t)pl.N);
    ep->off_R = ws.take(sizeof(double) * (size_t)pl.B);
    ep->total = ws.at;
    return RNNT_STATUS_SUCCESS;
}

// new = q * self + p * neighbour + c: the convex mix of the blank arc (log-weight x, cost cx) and the label arc (y, cy);
// the smaller weight is e / (1 + e), the other one 1 minus it (they sum to exactly 1); both -inf: no path, all 0
inline void arc_mix(double x, double y, double cx, double cy, double &q, double &pw, double &c) {
    if (x == kNegInf && y == kNegInf) {
        q = pw = c = 0.0;
        return;
    }
    const double e = std::exp(-std::fabs(x - y));
    const double wl = e / (1.0 + e);
    const bool ybig = y > x;
    pw = ybig ? 1.0 - wl : wl;
    q = ybig ? wl : 1.0 - wl;
    c = (q != 0.0 ? q * cx : 0.0) + (pw != 0.0 ? pw * cy : 0.0);
}

// A(t, .) for t = 0 .. T-1 (bwd: Bk(t, .) for t = T-1 .. 0) of one utterance; returns A(T-1, S) (bwd: Bk(0, 0))
double expect_utt(const mrnnt_problem *p, const CpuPlan &pl, const Views &w, double *out, const float *wb,
                  const float *we, int b, bool bwd) {
    const int T = p->T_host[b], S = p->S_host[b], W = S + 1;
    const int64_t r0 = pl.row_off[b], c0 = pl.col_off[b];
    const double *state = (bwd ? w.beta : w.alpha) + r0;
    double *O = out + r0;
    const int first = bwd ? T - 1 : 0;
    for (int i = 0; i < T; ++i) {
        const int t = bwd ? T - 1 - i : i;
        int lo_c, hi_c, lo_o, hi_o;
        state_band(w, c0, T, S, bwd ? t : t + 1, lo_c, hi_c);
        state_band(w, c0, T, S, bwd ? t + 1 : t, lo_o, hi_o);
        const bool edge = t == first;
        const int to = bwd ? std::min(t + 1, T - 1) : std::max(t - 1, 0);  // the other end's frame (not read at the edge)
        const double *st = state + (int64_t)to * W;
        const double *prev = O + (int64_t)to * W;
        const double *pb = w.lpb + r0 + (int64_t)t * W, *pe = w.lpe + r0 + (int64_t)t * W;
        const int64_t a0 = acts_row(pl, b, t, W);
        double *o = O + (int64_t)t * W;
        for (int s = 0; s < W; ++s) {
            if (s < lo_c || s > hi_c) {
                o[s] = 0.0;
                continue;
            }
            const int sn = bwd ? s + 1 : s - 1, se = bwd ? s : s - 1;
            const bool okx = s >= lo_o && s <= hi_o;
            const bool oky = sn >= lo_o && sn <= hi_o && (bwd ? s < S : s > 0);
            const double x = okx ? (edge ? 0.0 : st[s]) + pb[s] : kNegInf;
            const double y = oky ? (edge ? 0.0 : st[sn]) + pe[se] : kNegInf;
            double q, pw, c;
            arc_mix(x, y, (okx && wb) ? (double)wb[a0 + s] : 0.0, (oky && we) ? (double)we[a0 + se] : 0.0, q, pw, c);
            o[s] = q * (edge ? 0.0 : prev[s]) + pw * ((edge || !oky) ? 0.0 : prev[sn]) + c;
        }
    }
    return bwd ? O[0] : O[(int64_t)(T - 1) * W + S];
}

// The expected-cost gradient (mrnnt_cpu_expect_backward; the HIP path's ExpectRows / HatExpectRows, mrnnt_expect.hip):
// with pb / pe the arc posteriors of the row and A / Bk the cost states before and behind the arc,
//   W = posterior * (grad_costs - grad_expected * (A(t-1, s) + arc cost + Bk behind the arc - R))
// per arc. A row outside the band, below the occupancy threshold, or with both weights zero in fp32 is exact zeros
// (NaN without a finite ll).
struct ExpectWeights : RowsBase {
    const float *blank_cost, *label_cost, *grad_expected, *grad_costs;
    const double *A, *Bk, *Rv;
    struct Col : ArcState {
        double R, ge, gc;
        bool fin, last;
    };
    Col column(int64_t, int b, int t, int T, int S) const {
        const ArcState band(pl, w, b, t, T, S);
        return {band, Rv[b], grad_expected ? (double)grad_expected[b] : 0.0, grad_costs ? (double)grad_costs[b] : 0.0,
                std::isfinite(band.ll), t == T - 1};
    }
    bool weights(const Col &col, int s, int64_t r, int64_t a, double &Wb, double &We, float &fill) const {
        const int t = col.t, W = col.W;
        Wb = We = 0.0;
        if (col.fin && col.in_band(s)) {
            const double bs = col.alpha_in(s) - col.ll;
            if (!(bs + col.beta_at(s) < mrnnt::kDeadLogOcc)) {
                const double pb = std::exp(w.lpb[r] + bs + col.beta_blank(s));
                const double pe = (s < col.S) ? std::exp(w.lpe[r] + bs + col.beta_label(s)) : 0.0;
                const double ap = (t == 0) ? 0.0 : A[r - W];
                if (pb != 0.0)
                    Wb = pb * (col.gc - col.ge * (ap + (blank_cost ? (double)blank_cost[a] : 0.0) +
                                                  (col.last ? 0.0 : Bk[r + W]) - col.R));
                if (pe != 0.0)
                    We = pe * (col.gc - col.ge * (ap + (label_cost ? (double)label_cost[a] : 0.0) +
                                                  (col.last ? 0.0 : Bk[r + W + 1]) - col.R));
            }
        }
        fill = col.fin ? 0.0f : std::numeric_limits<float>::quiet_NaN();
        return !((float)Wb == 0.0f && (float)We == 0.0f);
    }
};
using ExpectRows = WeightedRows<ExpectWeights, weight_row>;
using HatExpectRows = WeightedRows<ExpectWeights, hat_weight_row>;

}  // namespace

extern "C" {

RNNTStatus mrnnt_cpu_expect_workspace_size(const mrnnt_problem *p, size_t *bytes) {
    return plan_bytes<CpuExpectPlan>(bytes, [&](CpuExpectPlan *ep) { return make_cpu_expect_plan(p, ep); });
}

// mrnnt_cpu_expect_forward / mrnnt_cpu_hat_expect_forward
static RNNTStatus cpu_expect_forward_impl(const mrnnt_problem *p, void *ws, size_t ws_bytes, const float *blank_cost,
                                          const float *label_cost, float *expected, float *costs, int with_grad,
                                          int num_threads, bool hat) {
    CpuExpectPlan ep;
    RNNTStatus st = make_cpu_expect_plan(p, &ep);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const CpuPlan &pl = ep.pl;
    if ((st = check_workspace(ws, ws_bytes, ep.total)) != RNNT_STATUS_SUCCESS) return st;
    if ((st = cpu_forward_impl(p, ws, ws_bytes, costs, with_grad ? 1 : 0, num_threads, hat)) != RNNT_STATUS_SUCCESS)
        return st;
    const Views w = views(pl, ws);
    double *A = ep.view(ws, ep.off_A), *Bk = ep.view(ws, ep.off_Bk), *R = ep.view(ws, ep.off_R);
    const int nt = threads_of(num_threads);
    const int dirs = with_grad ? 2 : 1;
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt)
    for (int i = 0; i < pl.B * dirs; ++i) {
        const int b = i / dirs;
        if (i % dirs == 0) {
            R[b] = expect_utt(p, pl, w, A, blank_cost, label_cost, b, false);
            if (expected) expected[b] = std::isfinite(w.ll[b]) ? (float)R[b] : std::numeric_limits<float>::quiet_NaN();
        } else {
            expect_utt(p, pl, w, Bk, blank_cost, label_cost, b, true);
        }
    }
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_cpu_expect_forward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const float *blank_cost,
                                    const float *label_cost, float *expected, float *costs, int with_grad,
                                    int num_threads) {
    return cpu_expect_forward_impl(p, ws, ws_bytes, blank_cost, label_cost, expected, costs, with_grad, num_threads,
                                   false);
}

RNNTStatus mrnnt_cpu_hat_expect_forward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const float *blank_cost,
                                        const float *label_cost, float *expected, float *costs, int with_grad,
                                        int num_threads) {
    return cpu_expect_forward_impl(p, ws, ws_bytes, blank_cost, label_cost, expected, costs, with_grad, num_threads,
                                   true);
}

// mrnnt_cpu_expect_backward / mrnnt_cpu_hat_expect_backward
static RNNTStatus cpu_expect_backward_impl(const mrnnt_problem *p, void *ws, size_t ws_bytes, const float *blank_cost,
                                           const float *label_cost, const float *grad_expected,
                                           const float *grad_costs, float *grads, int num_threads, bool hat) {
    CpuExpectPlan ep;
    RNNTStatus st = make_cpu_expect_plan(p, &ep);
    if (st != RNNT_STATUS_SUCCESS) return st;
    const CpuPlan &pl = ep.pl;
    if (!p->acts) return set_error(RNNT_STATUS_INVALID_VALUE, "acts is null");
    if (pl.S_max > 0 && !p->labels) return set_error(RNNT_STATUS_INVALID_VALUE, "labels is null");
    if (!grads) return set_error(RNNT_STATUS_INVALID_VALUE, "grads is null");
    if ((st = check_workspace(ws, ws_bytes, ep.total)) != RNNT_STATUS_SUCCESS) return st;
    const Views w = views(pl, ws);
    const int nt = threads_of(num_threads);
    const ExpectWeights x{{p, pl, w}, blank_cost, label_cost, grad_expected, grad_costs,
                          ep.view(ws, ep.off_A), ep.view(ws, ep.off_Bk), ep.view(ws, ep.off_R)};
    if (hat) grad_pass(HatExpectRows{x}, grads, nt);
    else grad_pass(ExpectRows{x}, grads, nt);
    return RNNT_STATUS_SUCCESS;
}

RNNTStatus mrnnt_cpu_expect_backward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const float *blank_cost,
                                     const float *label_cost, const float *grad_expected, const float *grad_costs,
                                     float *grads, int num_threads) {
    return cpu_expect_backward_impl(p, ws, ws_bytes, blank_cost, label_cost, grad_expected, grad_costs, grads,
                                    num_threads, false);
}

RNNTStatus mrnnt_cpu_hat_expect_backward(const mrnnt_problem *p, void *ws, size_t ws_bytes, const float *blank_cost,
                                         const float *label_cost, const float *grad_expected, const float *grad_costs,
                                         float *grads, int num_threads) {
    return cpu_expect_backward_impl(p, ws, ws_bytes, blank_cost, label_cost, grad_expected, grad_costs, grads,
                                    num_threads, true);
}

}  // extern "C"

// =================================================================================================
// reference-shaped C++ surface (reference include/cpu_workspace_manager.h, include/cpu_rnnt.h)

struct mrnnt_cpu_ws_state {
    const float *acts;
    const int *labels;
    int B, V;
    std::vector<int> T, S;
    std::vector<int64_t> row_off, col_off;  // lattice row / column offsets (row_off[b] + t (S_b+1) + s)
    int S_max = 0, T_max = 0;
    void *workspace = nullptr;
    bool owned = false;
    std::vector<int> alignment;  // copied by restrict_to_alignment, row stride max(T)
    bool restricted = false;
    int max_shift = 0;
    int align_blank = 0;
    std::vector<int> min_s, max_s;  // band per lattice column: the reference's min/max_allowed_s_ (:51-56, :207-224)
    // views of the workspace's per-row state (set_workspace), and the band of the last computation
    float *den = nullptr;
    double *alpha = nullptr, *beta = nullptr;
    bool computed_restricted = false;
    std::vector<int> cmin_s, cmax_s;
};

namespace {

mrnnt_problem cpu_problem_of(const mrnnt_cpu_ws_state *s, int blank) {
    mrnnt_problem p;
    std::memset(&p, 0, sizeof(p));
    p.B = s->B;
    p.V = s->V;
    p.blank = blank;
    p.T_host = s->T.data();
    p.S_host = s->S.data();
    p.acts = s->acts;
    p.labels = s->labels;
    // the reference's strides: labels max(S) (cpu_workspace_manager.h:121), alignment max(T) (:208)
    p.label_stride = s->S_max;
    p.alignment = s->restricted ? s->alignment.data() : nullptr;
    p.align_stride = s->T_max;
    p.align_blank = s->align_blank;
    p.max_shift = s->max_shift;
    p.num_rows = -1;
    return p;
}

RNNTStatus cpu_compute(mrnnt_cpu_ws_state *s, int blank, int num_threads, float *costs, float *grads) {
    if (!costs) return set_error(RNNT_STATUS_INVALID_VALUE, "costs is null");
    if (!s->workspace) return set_error(RNNT_STATUS_INVALID_VALUE, "workspace not set (set_workspace/create_workspace)");
    const mrnnt_problem p = cpu_problem_of(s, blank);
    size_t bytes = 0;
    RNNTStatus st = mrnnt_cpu_workspace_size(&p, &bytes);
    if (st != RNNT_STATUS_SUCCESS) return st;
    st = mrnnt_cpu_forward(&p, s->workspace, bytes, costs, grads != nullptr, num_threads);
    if (st != RNNT_STATUS_SUCCESS) return st;
    s->computed_restricted = s->restricted;
    s->cmin_s = s->min_s;
    s->cmax_s = s->max_s;
    if (!grads) return st;
    return mrnnt_cpu_backward(&p, s->workspace, nullptr, grads, num_threads);
}

constexpr float kNegInfF = -std::numeric_limits<float>::infinity();
constexpr float kNaNF = std::numeric_limits<float>::quiet_NaN();

}  // namespace

CpuRNNTWorkspaceManager<float>::CpuRNNTWorkspaceManager(const float *const acts, const int *const labels, const int B,
                                                        const int *T, const int *S, const int V)
    : st_(new mrnnt_cpu_ws_state) {
    st_->acts = acts;
    st_->labels = labels;
    st_->B = B;
    st_->V = V;
    if (B > 0 && T && S) {
        st_->T.assign(T, T + B);
        st_->S.assign(S, S + B);
        st_->S_max = *std::max_element(S, S + B);
        st_->T_max = *std::max_element(T, T + B);
        st_->row_off.assign(B + 1, 0);
        st_->col_off.assign(B + 1, 0);
        for (int b = 0; b < B; ++b) {  // (invalid lengths are rejected by get_workspace_size; keep offsets sane)
            st_->row_off[b + 1] = st_->row_off[b] + (int64_t)std::max(0, T[b]) * (std::max(0, S[b]) + 1);
            st_->col_off[b + 1] = st_->col_off[b] + std::max(0, T[b]);
        }
        st_->min_s.assign(st_->col_off[B], 0);
        st_->max_s.resize(st_->col_off[B]);
        for (int b = 0; b < B; ++b)
            std::fill(st_->max_s.begin() + st_->col_off[b], st_->max_s.begin() + st_->col_off[b + 1], S[b]);
    }
}

CpuRNNTWorkspaceManager<float>::~CpuRNNTWorkspaceManager() {
    if (st_->owned) std::free(st_->workspace);
    delete st_;
}

RNNTStatus CpuRNNTWorkspaceManager<float>::get_workspace_size(size_t *size_bytes) const {
    if (st_->B <= 0 || (int)st_->T.size() != st_->B) return set_error(RNNT_STATUS_INVALID_VALUE, "B must be > 0");
    // an alignment may be registered later: size for the restricted layout so either works
    mrnnt_problem p = cpu_problem_of(st_, 0);
    int dummy = 0;
    p.alignment = &dummy;
    return mrnnt_cpu_workspace_size(&p, size_bytes);
}

void CpuRNNTWorkspaceManager<float>::set_workspace(void *workspace) {
    if (st_->owned && st_->workspace && st_->workspace != workspace) std::free(st_->workspace);
    st_->workspace = workspace;
    st_->owned = false;
    st_->den = nullptr;
    st_->alpha = st_->beta = nullptr;
    CpuPlan pl;  // the per-row state's offsets do not depend on the alignment (the band comes last)
    const mrnnt_problem p = cpu_problem_of(st_, 0);
    if (workspace && st_->B > 0 && make_cpu_plan(&p, &pl) == RNNT_STATUS_SUCCESS) {
        const Views w = views(pl, workspace);
        st_->den = w.den;
        st_->alpha = w.alpha;
        st_->beta = w.beta;
    }
}

RNNTStatus CpuRNNTWorkspaceManager<float>::create_workspace() {
    size_t bytes = 0;
    const RNNTStatus st = get_workspace_size(&bytes);
    if (st != RNNT_STATUS_SUCCESS) return st;
    void *w = std::malloc(std::max<size_t>(1, bytes));
    if (!w) return set_error(RNNT_STATUS_MEMOPS_FAILED, "malloc workspace");
    set_workspace(w);
    st_->owned = true;
    return RNNT_STATUS_SUCCESS;
}

void CpuRNNTWorkspaceManager<float>::free_workspace() {
    if (st_->owned) std::free(st_->workspace);
    st_->workspace = nullptr;
    st_->owned = false;
    st_->den = nullptr;
    st_->alpha = st_->beta = nullptr;
}

void CpuRNNTWorkspaceManager<float>::restrict_to_alignment(const int *const alignments, int max_shift, int blank_idx) {
    st_->alignment.assign(alignments, alignments + (size_t)st_->B * st_->T_max);
    st_->restricted = true;
    st_->max_shift = max_shift;
    st_->align_blank = blank_idx;
    for (int b = 0; b < st_->B && !st_->col_off.empty(); ++b)
        band_utt(st_->alignment.data() + (size_t)b * st_->T_max, st_->T[b], max_shift, blank_idx,
                 st_->min_s.data() + st_->col_off[b], st_->max_s.data() + st_->col_off[b]);
}

int CpuRNNTWorkspaceManager<float>::B() const { return st_->B; }
int CpuRNNTWorkspaceManager<float>::V() const { return st_->V; }
int CpuRNNTWorkspaceManager<float>::T(int b) const { return st_->T[b]; }
int CpuRNNTWorkspaceManager<float>::S(int b) const { return st_->S[b]; }

int CpuRNNTWorkspaceManager<float>::alpha_s_min(int b, int t) const {
    return std::max(st_->min_s[st_->col_off[b] + t], t - (st_->T[b] - 1 - st_->S[b]));
}
int CpuRNNTWorkspaceManager<float>::alpha_s_max(int b, int t) const {
    return std::min(st_->max_s[st_->col_off[b] + t], t + 1);
}
int CpuRNNTWorkspaceManager<float>::beta_s_min(int b, int t) const {
    return t == 0 ? 0 : std::max(st_->min_s[st_->col_off[b] + t - 1], t - (st_->T[b] - st_->S[b]));
}
int CpuRNNTWorkspaceManager<float>::beta_s_max(int b, int t) const {
    return t == 0 ? 0 : std::min(st_->max_s[st_->col_off[b] + t - 1], t);
}

int CpuRNNTWorkspaceManager<float>::label(int b, int s) const {
    return st_->labels[(int64_t)b * st_->S_max + s];
}

long long CpuRNNTWorkspaceManager<float>::act_index(int b, int t, int s, int v) const {
    return (st_->row_off[b] + (int64_t)t * (st_->S[b] + 1) + s) * (int64_t)st_->V + v;
}

float CpuRNNTWorkspaceManager<float>::act(int b, int t, int s, int v) const { return st_->acts[act_index(b, t, s, v)]; }

void CpuRNNTWorkspaceManager<float>::set_denom(int b, int t, int s, float value) { get_denom(b, t, s) = value; }

float &CpuRNNTWorkspaceManager<float>::get_denom(int b, int t, int s) {
    static thread_local float none;
    if (!st_->den) return none = kNaNF;
    const int T = st_->T[b], S = st_->S[b];
    const int64_t c = st_->col_off[b] + t, r = st_->row_off[b] + (int64_t)t * (S + 1) + s;
    // rows the last computation reduced: the band (and alignment window), as in softmax_pass / row_window
    Views band{};
    if (st_->computed_restricted && !st_->cmin_s.empty()) {
        band.min_s = st_->cmin_s.data();
        band.max_s = st_->cmax_s.data();
    }
    int lo, hi;
    row_window(band, c, t, T, S, lo, hi);
    if (s < lo || s > hi) {  // never read by the computation: reduce it now (the reference's pass covers every row)
        float m;
        double sum;
        row_max_sum(st_->acts + r * st_->V, st_->V, m, sum);
        st_->den[r] = (float)(-(double)m - std::log(sum));
    }
    return st_->den[r];
}

void CpuRNNTWorkspaceManager<float>::set_alpha(int b, int t, int s, float value) {
    if (st_->alpha) st_->alpha[st_->row_off[b] + (int64_t)t * (st_->S[b] + 1) + s] = value;
}

float CpuRNNTWorkspaceManager<float>::get_alpha(int b, int t, int s) const {
    // reference cpu_workspace_manager.h:161-181: virtual starts, alignment band, lattice band
    const int T = st_->T[b], S = st_->S[b];
    if (s == -1) return kNegInfF;
    if (t == -1) return s == 0 ? 0.0f : kNegInfF;
    const int64_t c = st_->col_off[b] + t;
    if (s < st_->min_s[c] || s > st_->max_s[c]) return kNegInfF;
    if (s > t + 1 || S - s > T - 1 - t) return kNegInfF;
    if (!st_->alpha) return kNaNF;
    return (float)st_->alpha[st_->row_off[b] + (int64_t)t * (S + 1) + s];
}

void CpuRNNTWorkspaceManager<float>::set_beta(int b, int t, int s, float value) {
    if (st_->beta) st_->beta[st_->row_off[b] + (int64_t)t * (st_->S[b] + 1) + s] = value;
}

float CpuRNNTWorkspaceManager<float>::get_beta(int b, int t, int s) {
    // reference cpu_workspace_manager.h:185-205
    const int T = st_->T[b], S = st_->S[b];
    if (s == S + 1) return kNegInfF;
    if (t == T) return s == S ? 0.0f : kNegInfF;
    const int64_t c = st_->col_off[b] + t;
    if (t > 0 && (s < st_->min_s[c - 1] || s > st_->max_s[c - 1])) return kNegInfF;
    if (s > t || S - s - 1 > T - 1 - t) return kNegInfF;
    if (!st_->beta) return kNaNF;
    return (float)st_->beta[st_->row_off[b] + (int64_t)t * (S + 1) + s];
}

CpuRNNTComputer<float>::CpuRNNTComputer(CpuRNNTWorkspaceManager<float> &workspace_manager, int blank, int num_threads)
    : workspace_manager_(workspace_manager), blank_(blank), num_threads_(num_threads) {}

RNNTStatus CpuRNNTComputer<float>::cost_and_grad(float *costs, float *grads) {
    if (!grads) return set_error(RNNT_STATUS_INVALID_VALUE, "grads is null");
    return cpu_compute(workspace_manager_.state(), blank_, num_threads_, costs, grads);
}

RNNTStatus CpuRNNTComputer<float>::cost(float *costs) {
    return cpu_compute(workspace_manager_.state(), blank_, num_threads_, costs, nullptr);
}
