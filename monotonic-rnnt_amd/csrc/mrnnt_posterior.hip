// mrnnt_posterior.hip -- arc posteriors of the lattice (mrnnt_posteriors, include/mrnnt.h): a read-out over the
// workspace of mrnnt_forward(with_beta = 1). For lattice row (b, t, s), with the boundary conventions of row_coef
// (mrnnt_device.h: alpha(-1, s) = [s == 0], beta(T, s) = [s == S]):
//   blank_post(t, s) = exp(alpha(t-1, s) + lpb(t, s) + beta(t+1, s)   - ll)
//   label_post(t, s) = exp(alpha(t-1, s) + lpe(t, s) + beta(t+1, s+1) - ll)   (s < S; 0 at s = S)
//   emit(b, t)       = sum_s label_post(t, s)
//   label_time(b, s) = sum_t t * label_post(t, s)                             (s < S)
// -- the gradient's per-row coefficients RowCoef::cb / ce, here in fp64 (the fp64 exp: 2 per row against the 16 + 16 +
// 8 + 8 bytes of state the row reads) and stored as fp32. It reads lp / alpha / beta / ll and the lengths only: no
// acts, no labels.
//
// Which rows are read. Only the cells the gradient reads are trustworthy in the workspace: for a row inside the
// monotonic band max(0, t - (T - S)) <= s <= min(t, S) these are alpha(t-1, s), beta(t, s), beta(t+1, s) and
// beta(t+1, s+1) (the lean recursion step leaves finite values in cells outside it, mrnnt_setup.hip). A row outside
// the band is 0 without a read. A row inside it is unreachable when alpha(t-1, s) or beta(t, s) is -inf (a
// restricting alignment band, masked logits): exactly 0, decided before lp is read -- the forward writes lp only for
// the rows it reduced (align_window) and the workspace is not initialised. An utterance whose ll is not finite has
// every value NaN (zero_row_value's convention, extended to ll = NaN / +inf).
//
// One launch of 16-wave workgroups in two roles that share nothing (so no hand-off between them), every sum in a fixed
// order with fp64 accumulators (bitwise reproducible; no atomics):
//   utterance workgroups (the first utt_x * utt_y, the longer ones): label_time, a sum along t at fixed s. A workgroup
//     takes (utterance, 16 consecutive s), its 64 groups of 16 lanes take the band's frames t = s + g, s + g + 64, ...
//     (each group reads 16 consecutive rows of a frame: whole 128-byte lines of alpha / beta), partial sums meet in LDS
//     and are added in group order. label_post is recomputed from the state, not read from the other role's output.
//     They also write what is not a lattice column: emit of frames t >= T_b (0), label_time of s >= S_b (-1), the
//     padding rows of the padded layout (0), NaN over every output when device-resident lengths failed validation,
//     and the status word of an utterance longer than an output stride.
//   column workgroups (the rest): one wave per lattice column, grid-stride, lanes along s (coalesced state reads and
//     per-row stores in the layout of acts, acts_col_base); emit is the lane-serial sum over s = lane, lane + 64, ...
//     then a wave butterfly.
#include <algorithm>

#include "mrnnt_device.h"

namespace mrnnt {

namespace {

constexpr int kTimeLanes = 16;   // consecutive label positions per utterance workgroup
constexpr int kTimeGroups = 64;  // groups of kTimeLanes lanes striding over the frames
constexpr int kUttThreads = kTimeLanes * kTimeGroups;

// The two arc posteriors of row (t, s) INSIDE the monotonic band of an utterance with a finite ll.
template <bool BLANK>
__device__ __forceinline__ void row_post(const DevProblem &p, int t, int T, int S, int s, int64_t row, double ll,
                                         double &bp, double &ep) {
    const int W = S + 1;
    bp = 0.0;
    ep = 0.0;
    const double am = alpha_prev(p, t, s, row, W);
    const double b0 = p.beta[row];
    if (am == NEG_INF_D || b0 == NEG_INF_D) return;  // unreachable: lp may be unwritten
    const Lp l = p.lp[row];
    const double base = am - ll;
    const bool last = t == T - 1;
    if (BLANK) {
        const double b1 = last ? (s == S ? 0.0 : NEG_INF_D) : p.beta[row + W];
        bp = exp(l.b + base + b1);
    }
    if (s < S) {
        const double b2 = last ? (s + 1 == S ? 0.0 : NEG_INF_D) : p.beta[row + W + 1];
        ep = exp(l.e + base + b2);
    }
}

__device__ __forceinline__ void raise_status(const DevProblem &p) {
    if (p.status_host)  // a plain system-scope store into the caller's host-mapped word (as the setup kernel's)
        __hip_atomic_store(p.status_host, (int)RNNT_STATUS_INVALID_VALUE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

constexpr int kWaves = kUttThreads / 64;

// Column role: workgroup `blk` of `nblk`, one lattice column per wave.
__device__ __forceinline__ void post_cols(const DevProblem &p, const PosteriorArgs &a, int blk, int nblk) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float nan = __builtin_nanf("");
    for (int64_t c = (int64_t)blk * kWaves + wave; c < p.num_cols; c += (int64_t)nblk * kWaves) {
        const ColRef k = col_ref(p, c);
        const int lo = max(0, k.t - (k.T - k.S));
        const int hi = min(k.t, k.S);
        const double ll = p.ll[k.b];
        const bool fin = __builtin_isfinite(ll);
        const int64_t arow = acts_col_base(p, k.b, k.t, k.rowc);
        double acc = 0.0;
        for (int s = lane; s <= k.S; s += 64) {
            double bp = 0.0, ep = 0.0;
            if (fin && s >= lo && s <= hi) {
                if (a.blank) row_post<true>(p, k.t, k.T, k.S, s, k.rowc + s, ll, bp, ep);
                else row_post<false>(p, k.t, k.T, k.S, s, k.rowc + s, ll, bp, ep);
            }
            if (a.blank) a.blank[arow + s] = fin ? (float)bp : nan;
            if (a.label) a.label[arow + s] = fin ? (float)ep : nan;
            acc += ep;
        }
        if (a.emit) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
            // an utterance longer than the row: NaN over the row (its utterance workgroup raises the status word)
            if (lane == 0 && k.t < a.emit_stride)
                a.emit[(int64_t)k.b * a.emit_stride + k.t] = (fin && k.T <= a.emit_stride) ? (float)acc : nan;
        }
    }
}

// Utterance role: workgroup (bx, by) of (nx, ny); x over label tiles (and the fills), y over utterances. ok = false:
// device-resident lengths failed validation, every output element as the host sized it is NaN.
__device__ __forceinline__ void post_utts(const DevProblem &p, const PosteriorArgs &a, bool ok, int64_t rows_host,
                                          int bx, int nx, int by, int ny, double (*part)[kTimeLanes]) {
    const int tid = threadIdx.x;
    const float nan = __builtin_nanf("");
    if (!ok) {
        const int64_t i0 = ((int64_t)by * nx + bx) * kUttThreads + tid;
        const int64_t step = (int64_t)nx * ny * kUttThreads;
        for (int64_t i = i0; i < rows_host; i += step) {
            if (a.blank) a.blank[i] = nan;
            if (a.label) a.label[i] = nan;
        }
        if (a.emit)
            for (int64_t i = i0; i < (int64_t)p.B * a.emit_stride; i += step) a.emit[i] = nan;
        if (a.ltime)
            for (int64_t i = i0; i < (int64_t)p.B * a.time_stride; i += step) a.ltime[i] = nan;
        return;
    }
    const int sl = tid & (kTimeLanes - 1), g = tid / kTimeLanes;
    const int64_t xi = (int64_t)bx * kUttThreads + tid, xn = (int64_t)nx * kUttThreads;
    for (int b = by; b < p.B; b += ny) {
        const int T = p.T[b], S = p.S[b], W = S + 1;
        const double ll = p.ll[b];
        const bool fin = __builtin_isfinite(ll);
        const bool t_over = a.emit && T > a.emit_stride, s_over = a.ltime && S > a.time_stride;
        if ((t_over || s_over) && bx == 0 && tid == 0) raise_status(p);
        if (a.emit)  // frames past the utterance
            for (int64_t t = T + xi; t < a.emit_stride; t += xn) a.emit[(int64_t)b * a.emit_stride + t] = 0.0f;
        if (p.pad_S1 && (a.blank || a.label)) {  // padding rows of the padded layout
            const int64_t n = p.pad_T * p.pad_S1;
            for (int64_t i = xi; i < n; i += xn) {
                const int64_t t = i / p.pad_S1;
                if (t < T && i - t * p.pad_S1 <= S) continue;
                if (a.blank) a.blank[(int64_t)b * n + i] = 0.0f;
                if (a.label) a.label[(int64_t)b * n + i] = 0.0f;
            }
        }
        if (!a.ltime) continue;
        float *__restrict__ out = a.ltime + (int64_t)b * a.time_stride;
        const int64_t row0 = p.row_off[b];
        for (int64_t s0 = (int64_t)bx * kTimeLanes; s0 < a.time_stride; s0 += (int64_t)nx * kTimeLanes) {
            const int64_t s = s0 + sl;
            if (s0 >= S || s_over || !fin) {  // (uniform over the workgroup) nothing to sum
                if (g == 0 && s < a.time_stride) out[s] = s < S ? nan : -1.0f;
                continue;
            }
            double acc = 0.0;
            if (s < S) {  // frames with (t, s) inside the band: s <= t <= s + (T - S) (<= T - 1 as s < S)
                const int si = (int)s;
                for (int t = si + g; t <= si + (T - S); t += kTimeGroups) {
                    double bp, ep;
                    row_post<false>(p, t, T, S, si, row0 + (int64_t)t * W + si, ll, bp, ep);
                    acc += (double)t * ep;
                }
            }
            part[g][sl] = acc;
            __syncthreads();
            if (g == 0 && s < a.time_stride) {
                double sum = 0.0;
                for (int i = 0; i < kTimeGroups; ++i) sum += part[i][sl];
                out[s] = s < S ? (float)sum : -1.0f;
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kUttThreads) void posterior_kernel(DevProblem p, PosteriorArgs a, int utt_x, int utt_y) {
    __shared__ double part[kTimeGroups][kTimeLanes];
    const int64_t rows_host = p.pad_S1 ? (int64_t)p.B * p.pad_T * p.pad_S1 : p.num_rows;
    const bool ok = resolve_dyn(p);
    const int utt_blocks = utt_x * utt_y;
    if ((int)blockIdx.x < utt_blocks)
        post_utts(p, a, ok, rows_host, blockIdx.x % utt_x, utt_x, blockIdx.x / utt_x, utt_y, part);
    else if (ok)  // (failed validation: the utterance workgroups fill every output with NaN)
        post_cols(p, a, blockIdx.x - utt_blocks, gridDim.x - utt_blocks);
}

}  // namespace

hipError_t launch_posteriors(const DevProblem &p, const PosteriorArgs &a, int col_blocks, hipStream_t stream) {
    if (!a.blank && !a.label && !a.emit && !a.ltime) return hipSuccess;
    if (!a.blank && !a.label && !a.emit) col_blocks = 0;
    // utterance workgroups: x = the label tiles of label_time, and enough workgroups per utterance for the fills (4
    // elements per thread); y = the utterances
    const int64_t tiles = a.ltime ? (a.time_stride + kTimeLanes - 1) / kTimeLanes : 1;
    const int64_t fill = std::max<int64_t>(a.emit ? a.emit_stride : 0, (a.blank || a.label) ? p.pad_T * p.pad_S1 : 0);
    const int64_t fill_x = std::min<int64_t>(64, fill / (4 * kUttThreads));
    const int utt_x = (int)std::max<int64_t>(1, std::min<int64_t>(std::max(tiles, fill_x), 1024));
    const int utt_y = std::min(p.B, 65535);
    posterior_kernel<<<utt_x * utt_y + std::max(0, col_blocks), kUttThreads, 0, stream>>>(p, a, utt_x, utt_y);
    return hipGetLastError();
}

}  // namespace mrnnt
