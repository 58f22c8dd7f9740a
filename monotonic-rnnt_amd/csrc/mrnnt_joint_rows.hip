// mrnnt_joint_rows.hip -- the row lists of the fused joint (mrnnt_joint.hip): which lattice rows a pass visits, in
// column order, built on the device by a count / scan / write sequence; and the zeroing of what a shorter
// device-counted list leaves behind.
#include <algorithm>

#include "mrnnt_device.h"

namespace mrnnt {

// ---------------------------------------------------------------------------------------------------------
// row lists: entries (column, s) in column order, s ascending; mode 0 = in-band rows, 1 = live rows, 2 = path-live
// rows (mrnnt_joint_path_rows): the rows of the column's hull whose path weights Wb / We (p.alpha / p.beta after
// launch_path_coef) are not both zero, 3 = expect-live rows (mrnnt_joint_expect_rows): the rows of the monotonic band
// whose weights Wb / We (launch_expect_coef; the launch's p.alpha / p.beta point at them) are not both zero -- there is
// no hull, and a restricting alignment has already made the weights outside its window zero

__device__ __forceinline__ bool list_pred(const DevProblem &p, int mode, int t, int s, int64_t row, int W,
                                          double ll) {
    if (mode >= 2) return p.alpha[row] != 0.0 || p.beta[row] != 0.0;  // (NaN != 0: listed)
    if (mode == 0 || !p.occ_skip) return true;
    return row_live(alpha_prev(p, t, s, row, W) - ll + p.beta[row]);
}

template <bool WRITE>
__device__ __forceinline__ void row_list_column(const DevProblem &p, int mode, int64_t *__restrict__ cnt,
                                                int *__restrict__ lcol, int *__restrict__ ls, int64_t col, int lane) {
    const int b = p.col_b[col];
    const int T = p.T[b], S = p.S[b], W = S + 1;
    const int t = (int)(col - p.col_off[b]);
    const int64_t rowc = p.row_off[b] + (int64_t)t * W;
    int lo = max(0, t - (T - S)), hi = min(t, S);
    if (mode == 0) align_window(p, col, t, lo, hi);  // alignment-restricted: only the rows the recursion uses
    if (mode == 2) {
        // the hull rows as path_coef_kernel zeroed them and PathRows::column reads them (not align_window): Wb / We
        // outside are uninitialised and never looked at; a column without a valid path holds {kHullEmpty, -1}: no rows
        lo = max(lo, p.min_s[col] - 1);
        hi = min(hi, p.max_s[col]);
    }
    const double ll = mode == 1 ? p.ll[b] : 0.0;
    int64_t base = WRITE ? cnt[col] : 0;
    int n = 0;
    for (int s0 = lo; s0 <= hi; s0 += 64) {
        const int s = s0 + lane;
        const bool ok = s <= hi && list_pred(p, mode, t, s, rowc + s, W, ll);
        const unsigned long long mask = __ballot(ok);
        if (WRITE && ok) {
            const int rank = __popcll(mask & ((1ull << lane) - 1ull));
            lcol[base + rank] = (int)col;
            ls[base + rank] = s;
        }
        base += __popcll(mask);
        n += __popcll(mask);
    }
    if (!WRITE && lane == 0) cnt[col] = n;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void row_list_kernel(DevProblem p, int mode, int64_t *__restrict__ cnt,
                                                       int *__restrict__ lcol, int *__restrict__ ls) {
    const int lane = threadIdx.x & 63;
    // grid-stride over lattice columns (one per wave): the grid is capped, any number of columns works
    for (int64_t col = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); col < p.num_cols; col += (int64_t)gridDim.x * 4)
        row_list_column<WRITE>(p, mode, cnt, lcol, ls, col, lane);
}

// exclusive scan of a[0..n) in place, a[n] = total (n = lattice columns), in two launches over tiles of 1024: the
// tile sums (one workgroup per tile), then every workgroup adds the sums of the tiles before its own (<= a few
// hundred, one wave) and scans its tile through LDS. (A single workgroup walking all columns took ~130 us per list
// at the headline's 64,000 columns.)
constexpr int kScanTile = 1024;

__device__ __forceinline__ int64_t block_incl_scan1024(int64_t v, int64_t *wsum) {  // 1024 threads
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_incl_scan64(v);
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    if (wave == 0) {
        int64_t w = lane < 16 ? wsum[lane] : 0;
        w = wave_incl_scan64(w);
        if (lane < 16) wsum[lane] = w;
    }
    __syncthreads();
    return v + (wave > 0 ? wsum[wave - 1] : 0);
}

__global__ __launch_bounds__(1024) void scan_tiles_kernel(const int64_t *__restrict__ a, int64_t n,
                                                          int64_t *__restrict__ tile_sum) {
    __shared__ int64_t wsum[16];
    const int64_t i = (int64_t)blockIdx.x * kScanTile + threadIdx.x;
    const int64_t v = block_incl_scan1024(i < n ? a[i] : 0, wsum);
    if (threadIdx.x == kScanTile - 1) tile_sum[blockIdx.x] = v;
}

__global__ __launch_bounds__(1024) void scan_apply_kernel(int64_t *__restrict__ a, int64_t n,
                                                          const int64_t *__restrict__ tile_sum,
                                                          unsigned long long *__restrict__ total) {
    __shared__ int64_t wsum[16];
    __shared__ int64_t base;
    if (threadIdx.x < 64) {  // the tiles before this one, in order
        int64_t s = 0;
        for (int k = threadIdx.x; k < (int)blockIdx.x; k += 64) s += tile_sum[k];
        s = wave_incl_scan64(s);
        if (threadIdx.x == 63) base = s;
    }
    const int64_t i = (int64_t)blockIdx.x * kScanTile + threadIdx.x;
    const int64_t x = i < n ? a[i] : 0;
    const int64_t incl = block_incl_scan1024(x, wsum);  // (its barriers also publish `base`)
    if (i < n) a[i] = base + incl - x;
    if (i == n - 1 || (n == 0 && i == 0)) {
        a[n] = base + incl;
        if (total) *total = (unsigned long long)(base + incl);
    }
}

hipError_t launch_row_list(const DevProblem &p, int mode, int64_t *col_cnt, int *lcol, int *ls,
                           unsigned long long *total, hipStream_t stream) {
    const int64_t blocks = std::min<int64_t>((p.num_cols + 3) / 4, 1 << 20);
    row_list_kernel<false><<<(int)blocks, 256, 0, stream>>>(p, mode, col_cnt, lcol, ls);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the tile sums live past the counts (the workspace sizes col_cnt for it: joint_scan_scratch)
    const int64_t tiles = std::max<int64_t>(1, (p.num_cols + kScanTile - 1) / kScanTile);
    if (tiles > (1 << 20)) return hipErrorInvalidValue;
    int64_t *tile_sum = col_cnt + p.num_cols + 1;
    scan_tiles_kernel<<<(unsigned)tiles, 1024, 0, stream>>>(col_cnt, p.num_cols, tile_sum);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    scan_apply_kernel<<<(unsigned)tiles, 1024, 0, stream>>>(col_cnt, p.num_cols, tile_sum, total);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    row_list_kernel<true><<<(int)blocks, 256, 0, stream>>>(p, mode, col_cnt, lcol, ls);
    return hipGetLastError();
}

hipError_t launch_zero(void *ptr, size_t bytes, hipStream_t stream) { return hipMemsetAsync(ptr, 0, bytes, stream); }

// Rows [count, n) of G ([n, V] bf16) and Hact ([n, ld] bf16) as zeros, count = *count_dev (a device-counted live-row
// list sized by a host bound, JointArgs::n_dev): library GEMMs over all n rows then see zero rows there. Grid-stride
// 16-byte stores over the tail's byte range (rows are contiguous), 2-byte stores for its unaligned ends.
__global__ __launch_bounds__(256) void joint_tail_zero_kernel(unsigned short *__restrict__ G, int64_t gld,
                                                              unsigned short *__restrict__ Hact, int64_t hld, int64_t n,
                                                              const unsigned long long *__restrict__ count_dev) {
    const int64_t c = min((int64_t)*count_dev, n);
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    for (int which = 0; which < 2; ++which) {
        unsigned short *base = which ? Hact : G;
        const int64_t ld = which ? hld : gld;
        const int64_t e0 = c * ld, e1 = n * ld;  // elements
        const int64_t a0 = min(e1, (e0 + 7) / 8 * 8), a1 = max(a0, e1 / 8 * 8);
        if (tid < a0 - e0) base[e0 + tid] = 0;
        if (tid < e1 - a1) base[a1 + tid] = 0;
        for (int64_t o = a0 + tid * 8; o < a1; o += nth * 8) *reinterpret_cast<u4 *>(base + o) = u4{0u, 0u, 0u, 0u};
    }
}

hipError_t launch_joint_tail_zero(unsigned short *G, int V, unsigned short *Hact, int64_t hact_ld, int64_t n,
                                  const unsigned long long *count_dev, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    joint_tail_zero_kernel<<<2048, 256, 0, stream>>>(G, V, Hact, hact_ld, n, count_dev);
    return hipGetLastError();
}

}  // namespace mrnnt
