// mrnnt_joint_reduce.hip -- what follows the fused joint's gradient pass (mrnnt_joint.hip): the ordered dbias sums
// over its per-workgroup column sums, and the backward tail that folds dpre over the live rows into d_enc / d_pred.
#include <algorithm>
#include <type_traits>

#include "mrnnt_joint_tile.h"

namespace mrnnt {

#ifdef MRNNT_DEVTOOLS
// development build, joint_probe bit 4: the reduce's timeline -- thread 0 of the first kRedTraceWgs workgroups stamps
// [0] start, [1] setup done, [2 + 2f] frame f's rows summed, [3 + 2f] frame f's barriers passed (f < 6), [14] frame
// loop done, [15] flush done (s_memrealtime, 10 ns)
constexpr int kRedTraceWgs = 8192;
__device__ unsigned long long g_reduce_trace[kRedTraceWgs * 16];

int joint_reduce_trace(unsigned long long *out, int n) {
    n = std::min(n, kRedTraceWgs * 16);
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_reduce_trace), sizeof(unsigned long long) * n) != hipSuccess) return -1;
    return n;
}
#endif

// dbias += the column sums of the backward's per-workgroup rows, in a fixed order: stage 1 sums segments of
// kDbiasSeg rows (64 columns x 4 row lanes per workgroup, each lane its rows in order, the 4 lanes in order),
// stage 2 the segments in order. Bitwise reproducible, unlike float atomics (cdna_hip_programming.md Guideline 12).
constexpr int kDbiasSeg = 256;

__global__ __launch_bounds__(256) void dbias_seg_kernel(const float *__restrict__ part, int64_t nrows, int vpad,
                                                        float *__restrict__ seg_out) {
    __shared__ float red[4][64];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.y * kDbiasSeg, r1 = min(r0 + kDbiasSeg, nrows);
    float t = 0.0f;
    if (col < vpad)
        for (int64_t r = r0 + rl; r < r1; r += 4) t += part[r * vpad + col];
    red[rl][threadIdx.x & 63] = t;
    __syncthreads();
    if (rl == 0 && col < vpad)
        seg_out[(int64_t)blockIdx.y * vpad + col] = ((red[0][col & 63] + red[1][col & 63]) + red[2][col & 63]) +
                                                    red[3][col & 63];
}

__global__ __launch_bounds__(256) void dbias_total_kernel(const float *__restrict__ seg, int nseg, int vpad, int V,
                                                          float *__restrict__ dbias) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    float t = 0.0f;
    for (int k = 0; k < nseg; ++k) t += seg[(int64_t)k * vpad + v];
    dbias[v] += t;
}

int64_t joint_bwd_blocks(int64_t n) { return (n + 255) / 256; }  // the backward's workgroups (8 waves x 32 rows)

size_t joint_dbias_part_bytes(int64_t n_max, int V) {
    const int64_t nb = joint_bwd_blocks(n_max);
    return sizeof(float) * (size_t)vpad(V) * (size_t)(nb + (nb + kDbiasSeg - 1) / kDbiasSeg);
}

hipError_t launch_joint_dbias_sum(const JointArgs &j, int V, hipStream_t stream) {
    const int vp = vpad(V);
    const int64_t nb = joint_bwd_blocks(j.n);
    if (nb <= 0) return hipSuccess;
    const int64_t nseg = (nb + kDbiasSeg - 1) / kDbiasSeg;
    if (nseg > 65535) return hipErrorInvalidValue;
    float *seg = j.dbias_part + nb * vp;
    dbias_seg_kernel<<<dim3((vp + 63) / 64, (unsigned)nseg), 256, 0, stream>>>(j.dbias_part, nb, vp, seg);
    dbias_total_kernel<<<(V + 255) / 256, 256, 0, stream>>>(seg, (int)nseg, vp, V, j.dbias);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// backward tail: dpre = dH * (1 - Hact^2) over the live rows, summed into denc[b, t] (over s; written once per
// column) and dpred[b, s] (over t, accumulated in LDS frame by frame). One workgroup per (utterance, block of TT frames,
// slice of HS hidden units); 4 hidden units per thread (8-byte loads), 256/(HS/4) rows in flight. Bitwise
// reproducible: every sum has one fixed order and one writer -- a block's d_pred sums go to its own rows of a scratch
// buffer (part, with the label range it touched in rng) and pred_sum_kernel adds the blocks in block order; without
// scratch one block covers the whole utterance (TT = T_max) and flushes d_pred itself (fewer, longer workgroups).

constexpr int kReduceTT = 64;  // frames per workgroup (blocked form, and the sparse variant)

// SRC: where the tanh derivative's activation comes from.
//   kRedHact (default): read from Hact;
//   kRedTanh (development build, joint_reduce_hact = 0): recomputed, h = bf16(fast_tanh2(enc + pred)) exactly as the
//     gradient pass built it (same function and operands: the stored Hact's bits, test_joint_reduce_recomputed_
//     activation_is_bit_identical) -- enc[b, t] once per frame, the pred slice staged in LDS, so the reduce streams dH
//     alone (4 GB at H = 512 instead of 8). Measured slower, 2.71 -> 4.26 ms: the frame loop is latency-bound, and the
//     staged slice costs occupancy (three workgroups per CU instead of five) -- the bytes were not its limit;
//   kRedPre: dH already holds dpre = dH * (1 - Hact^2) (mrnnt_joint_dpre's epilogue).
constexpr int kRedTanh = 0, kRedHact = 1, kRedPre = 2;

// AP: LDS row pitch of the accumulators (HS + 1: a column's consecutive rows start on successive banks, so the four
// 4-byte accesses per thread -- 8 threads per row, 4 rows per 32-lane bank group -- are conflict-free; a pitch of HS
// put rows s and s + 2 on the same banks, SQ_LDS_BANK_CONFLICT 0.67 of the LDS cycles in round 4).
template <int HS, int SRC, int AP>
__global__ __launch_bounds__(256) void joint_reduce_kernel(DevProblem p, JointArgs j, const int64_t *__restrict__ off,
                                                           const unsigned short *__restrict__ dH,
                                                           float *__restrict__ d_enc, float *__restrict__ d_pred,
                                                           int tt, int ntb, int wstride, float *__restrict__ part,
                                                           int *__restrict__ rng) {
    constexpr int TPR = HS / 4;     // threads per row slice
    constexpr int RP = 256 / TPR;   // rows in parallel
    extern __shared__ float lds[];  // acc[(S_b+1) * AP], red[RP][AP], then (kRedTanh) pred slice [S_b+1][HS] bf16
    const int H = j.H;
    const int nh = H / HS;
    // the h-slices of one block of frames are consecutive workgroups: they read the same rows (L2 reuse)
    const int bx = blockIdx.x / nh;
    const int h0 = (blockIdx.x % nh) * HS;
    const int b = bx / ntb, blk = bx % ntb;
    const int t0 = blk * tt;
    const int T = p.T[b], S = p.S[b];
    const int tid = threadIdx.x;
    if (t0 >= T) {  // (past this utterance's frames: an empty label range for the block sum)
        if (part && h0 == 0 && tid == 0) {
            rng[2 * bx] = 1;
            rng[2 * bx + 1] = 0;
        }
        return;
    }
    const int hl = (tid % TPR) * 4, rsub = tid / TPR;
#ifdef MRNNT_DEVTOOLS
    const bool trace = (j.probe & 16) && blockIdx.x < (unsigned)kRedTraceWgs;
#define RED_MARK(i) \
    do { if (trace && tid == 0) g_reduce_trace[blockIdx.x * 16 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define RED_MARK(i) ((void)0)
#endif
    RED_MARK(0);
    float *acc = lds;
    float *red = lds + (S + 1) * AP;
    const int64_t tslots = j.enc_sb / H, sslots = j.pred_sb / H;
    const int t1 = min(t0 + tt, T);
    // label positions this block of frames touches: rows of a column are listed by ascending s, so the first and
    // last row of each column bound them (a few labels under an alignment restriction, the band otherwise); only
    // that slice of the d_pred accumulator is cleared and flushed (min / max: order-independent)
    __shared__ int srange[2];
    // the block's list offsets, read once here (kReduceTT frames): the frame loop then starts each frame's row loads
    // without first waiting for a global load of its offsets
    __shared__ int64_t soff[kReduceTT + 1];
    const bool staged_off = t1 - t0 <= kReduceTT && !(kVariants && (j.probe & 64));  // (probe bit 6: A/B)
    if (tid == 0) {
        srange[0] = S + 1;
        srange[1] = -1;
    }
    __syncthreads();
    for (int t = t0 + tid; t < t1; t += 256) {
        const int64_t col = p.col_off[b] + t;
        const int64_t r0 = off[col], r1 = off[col + 1];
        if (staged_off) {
            soff[t - t0] = r0;
            if (t == t1 - 1) soff[t1 - t0] = r1;
        }
        if (r1 > r0) {
            atomicMin(&srange[0], j.ls[r0]);
            atomicMax(&srange[1], j.ls[r1 - 1]);
        }
    }
    __syncthreads();
    const int s_lo = srange[0], s_hi = srange[1];
    for (int i = s_lo * HS + tid; i < (s_hi + 1) * HS; i += 256) acc[i / HS * AP + i % HS] = 0.0f;
    // kRedTanh: pred[b, s, h0 .. h0 + HS) for the touched s, 8 bytes per thread and row
    unsigned short *pl = reinterpret_cast<unsigned short *>(red + RP * AP);
    if constexpr (SRC == kRedTanh) {
        for (int i = s_lo * TPR + tid; i < (s_hi + 1) * TPR; i += 256) {
            const int ss = i / TPR, hq = (i % TPR) * 4;
            *reinterpret_cast<uint2 *>(pl + ss * HS + hq) =
                *reinterpret_cast<const uint2 *>(j.pred + (int64_t)b * j.pred_sb + (int64_t)ss * H + h0 + hq);
        }
    }
    __syncthreads();
    RED_MARK(1);
    for (int t = t0; t < t1; ++t) {
        const int64_t col = p.col_off[b] + t;
        const int64_t r0 = staged_off ? soff[t - t0] : off[col], r1 = staged_off ? soff[t - t0 + 1] : off[col + 1];
        float e0 = 0.0f, e1 = 0.0f, e2 = 0.0f, e3 = 0.0f;
        uint2 ev = make_uint2(0u, 0u);
        if constexpr (SRC == kRedTanh)
            if (r1 > r0) ev = *reinterpret_cast<const uint2 *>(j.enc + (int64_t)b * j.enc_sb + (int64_t)t * H + h0 + hl);
        for (int64_t r = r0 + rsub; r < r1; r += RP) {
            const int s = j.ls[r];
            const uint2 dv = *reinterpret_cast<const uint2 *>(dH + r * H + h0 + hl);
            float v0 = bf16_lo(dv.x), v1 = bf16_hi(dv.x), v2 = bf16_lo(dv.y), v3 = bf16_hi(dv.y);
            if constexpr (SRC != kRedPre) {
                float h_0, h_1, h_2, h_3;
                if constexpr (SRC == kRedHact) {
                    const uint2 hv = *reinterpret_cast<const uint2 *>(j.Hact + r * j.hact_ld + h0 + hl);
                    h_0 = bf16_lo(hv.x), h_1 = bf16_hi(hv.x), h_2 = bf16_lo(hv.y), h_3 = bf16_hi(hv.y);
                } else {  // build_row's activation, bit for bit
                    const uint2 pv = *reinterpret_cast<const uint2 *>(pl + s * HS + hl);
                    const f2 ya = fast_tanh2((f2){bf16_lo(ev.x), bf16_hi(ev.x)} + (f2){bf16_lo(pv.x), bf16_hi(pv.x)});
                    const f2 yb = fast_tanh2((f2){bf16_lo(ev.y), bf16_hi(ev.y)} + (f2){bf16_lo(pv.y), bf16_hi(pv.y)});
                    h_0 = (float)(__bf16)ya.x, h_1 = (float)(__bf16)ya.y, h_2 = (float)(__bf16)yb.x;
                    h_3 = (float)(__bf16)yb.y;
                }
                v0 *= 1.0f - h_0 * h_0;
                v1 *= 1.0f - h_1 * h_1;
                v2 *= 1.0f - h_2 * h_2;
                v3 *= 1.0f - h_3 * h_3;
            }
            e0 += v0;
            e1 += v1;
            e2 += v2;
            e3 += v3;
            float *a = acc + s * AP + hl;  // distinct s within a column: one writer per element
            a[0] += v0;
            a[1] += v1;
            a[2] += v2;
            a[3] += v3;
        }
        if (kVariants && (j.probe & 4)) {  // development timing probe: no frame barriers / d_enc sum (wrong results)
            if (rsub == 0) {
                float *de = d_enc + ((int64_t)b * tslots + t) * H + h0 + hl;
                de[0] = e0;
                de[1] = e1;
                de[2] = e2;
                de[3] = e3;
            }
            continue;
        }
        if (t - t0 < 6) RED_MARK(2 + 2 * (t - t0));
        float *rr = red + rsub * AP + hl;
        rr[0] = e0;
        rr[1] = e1;
        rr[2] = e2;
        rr[3] = e3;
        __syncthreads();
        if (tid < HS) {
            float sum = 0.0f;
#pragma unroll 4
            for (int g = 0; g < RP; ++g) sum += red[g * AP + tid];
            d_enc[((int64_t)b * tslots + t) * H + h0 + tid] = sum;
        }
        __syncthreads();
        if (t - t0 < 6) RED_MARK(3 + 2 * (t - t0));
    }
    RED_MARK(14);
    if (!part) {  // one block per utterance: this workgroup is the one writer
        for (int i = s_lo * HS + tid; i < (s_hi + 1) * HS; i += 256)
            d_pred[((int64_t)b * sslots + i / HS) * H + h0 + i % HS] += acc[i / HS * AP + i % HS];
        return;
    }
    float *pb = part + (int64_t)bx * wstride * H;
    for (int i = s_lo * HS + tid; i < (s_hi + 1) * HS; i += 256)
        pb[(int64_t)(i / HS) * H + h0 + i % HS] = acc[i / HS * AP + i % HS];
    if (h0 == 0 && tid == 0) {
        rng[2 * bx] = s_lo;
        rng[2 * bx + 1] = s_hi;
    }
    RED_MARK(15);
#undef RED_MARK
}

// d_pred[b, s, :] += the blocks' sums of label position s, in block order (the blocks whose range holds s)
__global__ __launch_bounds__(256) void pred_sum_kernel(DevProblem p, const float *__restrict__ part,
                                                       const int *__restrict__ rng, int ntb, int wstride, int H,
                                                       int64_t sslots, float *__restrict__ d_pred) {
    const int b = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int s = (int)(e / H), h = (int)(e % H);
    if (s > p.S[b]) return;
    float t = 0.0f;
    for (int k = 0; k < ntb; ++k) {
        const int bx = b * ntb + k;
        if (s >= rng[2 * bx] && s <= rng[2 * bx + 1]) t += part[((int64_t)bx * wstride + s) * H + h];
    }
    d_pred[((int64_t)b * sslots + s) * H + h] += t;
}

size_t joint_reduce_scratch_bytes(int B, int T_max, int S_max, int H) {
    const int64_t ntb = (T_max + kReduceTT - 1) / kReduceTT;
    return sizeof(float) * (size_t)B * ntb * (S_max + 1) * H + sizeof(int) * 2 * (size_t)B * ntb + 256;
}

// Sparse variant (development build, joint_reduce_sparse = 2; float atomics: not bitwise reproducible) (few live rows per frame, e.g. alignment-restricted training): the rows of a block of frames are
// processed all at once (TPR threads per row) instead of frame by frame, so a workgroup does not wait one
// dependent load chain per frame; d_enc and d_pred partials meet in LDS through ds_add_f32.
template <int HS>
__global__ __launch_bounds__(256) void joint_reduce_sparse_kernel(DevProblem p, JointArgs j,
                                                                  const int64_t *__restrict__ off,
                                                                  const unsigned short *__restrict__ dH,
                                                                  float *__restrict__ d_enc, float *__restrict__ d_pred,
                                                                  int ntb) {
    constexpr int TPR = HS / 4;
    constexpr int RP = 256 / TPR;
    extern __shared__ float lds[];  // acc_pred[(S_b+1) * HS] then acc_enc[kReduceTT * HS]
    const int H = j.H;
    const int nh = H / HS;
    const int bx = blockIdx.x / nh;
    const int h0 = (blockIdx.x % nh) * HS;
    const int b = bx / ntb;
    const int t0 = (bx % ntb) * kReduceTT;
    const int T = p.T[b], S = p.S[b];
    if (t0 >= T) return;
    const int tid = threadIdx.x;
    const int hl = (tid % TPR) * 4, rsub = tid / TPR;
    const int t1 = min(t0 + kReduceTT, T);
    float *accp = lds;
    float *acce = lds + (S + 1) * HS;
    const int64_t c0 = p.col_off[b];
    const int64_t rb = off[c0 + t0], re = off[c0 + t1];
    // the label range the rows touch: only that slice of the d_pred accumulator is cleared and flushed
    __shared__ int srange[2];
    if (tid == 0) {
        srange[0] = S + 1;
        srange[1] = -1;
    }
    for (int i = tid; i < kReduceTT * HS; i += 256) acce[i] = 0.0f;
    __syncthreads();
    for (int64_t r = rb + tid; r < re; r += 256) {
        const int s = j.ls[r];
        atomicMin(&srange[0], s);
        atomicMax(&srange[1], s);
    }
    __syncthreads();
    const int s_lo = srange[0], s_hi = srange[1];
    for (int i = s_lo * HS + tid; i < (s_hi + 1) * HS; i += 256) accp[i] = 0.0f;
    __syncthreads();
    for (int64_t r = rb + rsub; r < re; r += RP) {
        const int s = j.ls[r];
        const int tt = (int)(j.lcol[r] - c0 - t0);
        const uint2 dv = *reinterpret_cast<const uint2 *>(dH + r * H + h0 + hl);
        const uint2 hv = *reinterpret_cast<const uint2 *>(j.Hact + r * j.hact_ld + h0 + hl);
        const float h_0 = bf16_lo(hv.x), h_1 = bf16_hi(hv.x), h_2 = bf16_lo(hv.y), h_3 = bf16_hi(hv.y);
        const float v[4] = {bf16_lo(dv.x) * (1.0f - h_0 * h_0), bf16_hi(dv.x) * (1.0f - h_1 * h_1),
                            bf16_lo(dv.y) * (1.0f - h_2 * h_2), bf16_hi(dv.y) * (1.0f - h_3 * h_3)};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            atomicAdd(&acce[tt * HS + hl + q], v[q]);
            atomicAdd(&accp[s * HS + hl + q], v[q]);
        }
    }
    __syncthreads();
    const int64_t tslots = j.enc_sb / H, sslots = j.pred_sb / H;
    for (int i = tid; i < (t1 - t0) * HS; i += 256)  // rows (b, t < T_b) of d_enc are overwritten (ABI)
        d_enc[((int64_t)b * tslots + t0 + i / HS) * H + h0 + i % HS] = acce[i];
    for (int i = s_lo * HS + tid; i < (s_hi + 1) * HS; i += 256) {
        const float v = accp[i];
        if (v != 0.0f) atomicAdd(&d_pred[((int64_t)b * sslots + i / HS) * H + h0 + i % HS], v);
    }
}

hipError_t launch_joint_reduce(const DevProblem &p, const JointArgs &j_in, const int64_t *off, int T_max, int S_max,
                               const unsigned short *dH, float *d_enc, float *d_pred, void *scratch,
                               size_t scratch_bytes, hipStream_t stream) {
    JointArgs j = j_in;
    if (kVariants) j.probe = tuning().joint_probe;
    const int ntb = (T_max + kReduceTT - 1) / kReduceTT;
    const int W = S_max + 1;
    // the row-parallel sparse kernel with float atomics: development A/B only (joint_reduce_sparse = 2; dH + Hact)
    const bool pre = j.Hact == nullptr;  // dH holds dpre (mrnnt_joint_dpre)
    const bool sparse = kVariants && tuning().joint_reduce_sparse == 2 && !pre;
    const bool tanh_src = kVariants && tuning().joint_reduce_hact == 0 && !pre;
    auto go = [&](auto hs_tag) -> hipError_t {
        constexpr int HS = decltype(hs_tag)::value;
        // (accumulator pitch HS + 1; the development build's joint_reduce_pad = 0 runs pitch HS, bit-identical)
        constexpr int AP = HS + 1;
        const bool nopad = kVariants && tuning().joint_reduce_pad == 0;
        auto kern = pre ? (nopad ? joint_reduce_kernel<HS, kRedPre, HS> : joint_reduce_kernel<HS, kRedPre, AP>)
                        : (tanh_src ? joint_reduce_kernel<HS, kRedTanh, AP>
                                    : (nopad ? joint_reduce_kernel<HS, kRedHact, HS>
                                             : joint_reduce_kernel<HS, kRedHact, AP>));
        const int apitch = nopad ? HS : AP;
        if (sparse) {
            const size_t lds = sizeof(float) * ((size_t)W * HS + (size_t)kReduceTT * HS);
            joint_reduce_sparse_kernel<HS><<<p.B * ntb * (j.H / HS), 256, lds, stream>>>(p, j, off, dH, d_enc,
                                                                                          d_pred, ntb);
            return hipSuccess;
        }
        // (+ the staged pred slice, bf16 [W][HS], of the recomputing form: up to 88 KiB)
        const size_t lds = sizeof(float) * ((size_t)W * apitch + 256 / (HS / 4) * apitch) +
                           (tanh_src ? sizeof(unsigned short) * W * HS : 0);
        const hipError_t ea = allow_lds(kern, lds);
        if (ea != hipSuccess) return ea;
        if (scratch && scratch_bytes >= joint_reduce_scratch_bytes(p.B, T_max, S_max, j.H)) {
            // blocks of kReduceTT frames, their d_pred sums added in block order by pred_sum_kernel
            float *part = static_cast<float *>(scratch);
            int *rng = reinterpret_cast<int *>(part + (size_t)p.B * ntb * W * j.H);
            kern<<<p.B * ntb * (j.H / HS), 256, lds, stream>>>(p, j, off, dH, d_enc, d_pred, kReduceTT, ntb, W, part,
                                                                rng);
            pred_sum_kernel<<<dim3((unsigned)(((int64_t)W * j.H + 255) / 256), (unsigned)p.B), 256, 0, stream>>>(
                p, part, rng, ntb, W, j.H, j.pred_sb / j.H, d_pred);
        } else {  // one block per utterance (no scratch)
            kern<<<p.B * (j.H / HS), 256, lds, stream>>>(p, j, off, dH, d_enc, d_pred, T_max, 1, W, nullptr, nullptr);
        }
        return hipSuccess;
    };
    if ((int64_t)p.B * ntb * (j.H / 4) > (1ll << 24)) return hipErrorInvalidValue;  // 32-bit dispatch size
    // LDS = W * HS fp32 + 4 KiB + W * HS bf16: about 43 KiB at the headline (three workgroups per CU), <= 88 KiB
    const hipError_t e = W <= 448    ? go(std::integral_constant<int, 32>())
                         : W <= 896  ? go(std::integral_constant<int, 16>())
                         : W <= 1792 ? go(std::integral_constant<int, 8>())
                                     : go(std::integral_constant<int, 4>());
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace mrnnt
