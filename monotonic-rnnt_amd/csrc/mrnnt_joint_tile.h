// mrnnt_joint_tile.h -- the device-side pieces the fused joint's kernel units share (mrnnt_joint.hip: the forward and
// gradient passes; mrnnt_joint_reduce.hip: the d_enc / d_pred reduce): the packed-f32 helpers and the fast tanh, a list
// row's position and activations, the W chunk in LDS as MFMA tiles (WTile: 32x32x16, WTile16: 16x16x32), the chunk loop
// and the register picks of its epilogues. The tiling itself is described at the top of mrnnt_joint.hip.
// Not installed; not part of the ABI.
#pragma once

#include "mrnnt_device.h"

namespace mrnnt {

#ifdef MRNNT_DEVTOOLS
// development build: the forward's per-wave timeline (s_memrealtime ticks) for every wave (8) of the first
// kJointTraceWgs workgroups, 8 marks each: start, bias staged, activations built, first chunk done, end, and inside
// chunk 0: after the DMA wait, after the barrier, after the MFMAs (defined in mrnnt_joint.hip, beside its reader)
constexpr int kJointTraceWgs = 4096;
extern __device__ unsigned long long g_joint_trace[kJointTraceWgs * 64];
#define JOINT_MARK(i)                                                                                         \
    do {                                                                                                      \
        if ((threadIdx.x & 63) == 0 && blockIdx.x < (unsigned)kJointTraceWgs && threadIdx.x < 512)            \
            g_joint_trace[blockIdx.x * 64 + (threadIdx.x >> 6) * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define JOINT_MARK(i) ((void)0)
#endif
#define FWD_MARK(i)                 \
    do {                            \
        if constexpr (TR) JOINT_MARK(i); \
    } while (0)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f2 __attribute__((ext_vector_type(2)));

// the vocabulary padded to whole 32-entry chunks: the bias rows in LDS, the dbias column sums
__host__ __device__ constexpr int vpad(int V) { return (V + 31) / 32 * 32; }

// scalar f32 in the MFMA loop's epilogue: a packed v_pk_fma/add_f32 beside MFMAs costs more issue time than the
// two scalar ops it replaces (MI355X_MICROARCH.md, per-instruction constants; the joint file is built with
// -fno-slp-vectorize so these stay scalar -- measured 2 % faster forward and backward than packed)
__device__ __forceinline__ f2 add2(f2 a, f2 b) { return (f2){a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ f2 mul2(f2 a, f2 b) { return (f2){a.x * b.x, a.y * b.y}; }
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return (f2){fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y)}; }

__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }


// tanh(x) = sign(x) (1 - e) / (1 + e), e = exp(-2|x|) (v_exp_f32 + v_rcp_f32, |error| ~ 1e-7), two at a time on
// packed f32 (v_pk_*): the build runs before the MFMA loop, where packing halves its VALU. (The form
// 1 - 2 / (1 + e^{2x}) has 39 % fewer non-transcendental VALU and measured 0.1-0.2 ms slower at H = 512:
// profiles/r02/joint/joint_tanh_rcp_ab.json.)
__device__ __forceinline__ f2 fast_tanh2(f2 x) {
    const f2 ax = {fabsf(x.x), fabsf(x.y)};
    const f2 t = ax * (f2){-2.0f * kLog2e, -2.0f * kLog2e};
    const f2 e = {fast_exp2(t.x), fast_exp2(t.y)};
    const f2 num = (f2){1.0f, 1.0f} - e, den = (f2){1.0f, 1.0f} + e;
    const f2 y = num * (f2){__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
    return (f2){copysignf(y.x, x.x), copysignf(y.y, x.y)};
}

// ---------------------------------------------------------------------------------------------------------
// the fused tile

struct RowPos {
    bool valid;
    int b, t, s, T, S, lab;
    int64_t row;  // packed lattice row
};

__device__ __forceinline__ int64_t list_len(const JointArgs &j) {
    return j.n_dev ? min((int64_t)*j.n_dev, j.n) : j.n;  // (a device count never reaches past the host bound)
}

__device__ __forceinline__ RowPos row_pos(const DevProblem &p, const JointArgs &j, int64_t i) {
    RowPos q{false, 0, 0, 0, 1, 0, -1, 0};
    if (i >= list_len(j)) return q;
    const int col = j.lcol[i];
    q.s = j.ls[i];
    q.b = p.col_b[col];
    q.t = (int)(col - p.col_off[q.b]);
    q.T = p.T[q.b];
    q.S = p.S[q.b];
    q.row = p.row_off[q.b] + (int64_t)q.t * (q.S + 1) + q.s;
    // -2: a label outside [0, V) (device labels are not range-checked on the host): no capture, lpe = NaN
    const int l = q.s < q.S ? p.labels[(int64_t)q.b * p.label_stride + q.s] : -1;
    q.lab = (q.s < q.S && (unsigned)l >= (unsigned)p.V) ? -2 : l;
    q.valid = true;
    return q;
}

// B operand of one row: h = bf16(tanh(enc[b,t] + pred[b,s])) for k = k0 + KSTEP ks + [0, 8), ks < NK; optionally
// stored to Hact. Invalid lanes (past the end of the list) read row 0 and zero the result: no branch around the loads
// (a branch per load makes hipcc wait vmcnt(0) after each one).
template <int NK, int KSTEP, bool STORE>
__device__ __forceinline__ void build_row(const JointArgs &j, const RowPos &q, int k0, int64_t i, bf16x8 *bfr) {
    constexpr int H = NK * KSTEP;
    const bool v = q.valid;
    const int t_ld = (kVariants && (j.probe & 2)) ? 0 : q.t, s_ld = (kVariants && (j.probe & 1)) ? 0 : q.s;
    const unsigned short *er = j.enc + (v ? (int64_t)q.b * j.enc_sb + (int64_t)t_ld * H : 0) + k0;
    const unsigned short *pr = j.pred + (v ? (int64_t)q.b * j.pred_sb + (int64_t)s_ld * H : 0) + k0;
    const float keep = v ? 1.0f : 0.0f;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
        const u4 ev = *reinterpret_cast<const u4 *>(er + KSTEP * ks);
        const u4 pv = *reinterpret_cast<const u4 *>(pr + KSTEP * ks);
        bf16x8 h;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const f2 y = fast_tanh2((f2){bf16_lo(ev[w]), bf16_hi(ev[w])} + (f2){bf16_lo(pv[w]), bf16_hi(pv[w])}) *
                         (f2){keep, keep};
            h[2 * w] = (__bf16)y.x;
            h[2 * w + 1] = (__bf16)y.y;
        }
        if (STORE && v) *reinterpret_cast<bf16x8 *>(j.Hact + i * j.hact_ld + KSTEP * ks + k0) = h;
        bfr[ks] = h;
    }
    if (STORE && v) {  // columns past H: a ones column (dbias from the dweight GEMM), then zeros
        for (int64_t c = H + k0; c < j.hact_ld; c += KSTEP) {
            bf16x8 e = {};
            if (c == H) e[0] = (__bf16)1.0f;
            *reinterpret_cast<bf16x8 *>(j.Hact + i * j.hact_ld + c) = e;
        }
    }
}

// 32x32x16 tile: lane l holds k = 16 ks + 8 (l >> 5) + [0, 8) of row l & 31
template <int KS, bool STORE>
__device__ __forceinline__ void build_act(const JointArgs &j, const RowPos &q, int half, int64_t i,
                                          bf16x8 (&bfr)[KS]) {
    build_row<KS, 16, STORE>(j, q, 8 * half, i, bfr);
}

// W chunk (32 vocabulary rows x H bf16) in LDS: unpadded, the 16-byte piece p of row r stored at piece
// p ^ (r & 15) (T2 XOR swizzle: the 16 lanes of a ds_read_b128 group read 16 distinct rows at one column and
// land on 16 distinct bank quads). Filled by LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave-instruction,
// lane-linear destination, so the swizzle goes on the per-lane SOURCE address) -- no staging registers.
template <int KS>
struct WTile {
    static constexpr int H = 16 * KS;
    static constexpr int CPR = H / 8;    // 16-byte pieces per row (a multiple of 16 for H % 128 == 0)
    static constexpr int NI = CPR / 2;   // wave-instructions per tile: 32 * CPR / 64
    static constexpr int ELEMS = 32 * H; // bf16 elements per tile

    // issue the DMA of vocabulary chunk c into wbuf (rows >= V read row V-1; the epilogue masks them); the NW
    // waves of the workgroup split the NI wave-instructions
    template <int NW>
    __device__ static __forceinline__ void stage(const JointArgs &j, int V, int c, unsigned short *wbuf) {
        static_assert(NI % NW == 0, "DMA instructions must split evenly over the waves");
        const int lane = threadIdx.x & 63;
        const int wave = (!kVariants || (j.opt & 1)) ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : threadIdx.x >> 6;
        if ((!kVariants || (j.opt & 1)) && 32 * c + 32 <= V) {
            // a whole chunk: a wave-uniform chunk base plus loop-invariant 32-bit lane offsets (no per-chunk 64-bit
            // address arithmetic or row clamp on the vector pipe; the last partial chunk takes the clamped form)
            const char *base = reinterpret_cast<const char *>(j.W + (int64_t)32 * c * H);
#pragma unroll
            for (int ii = 0; ii < NI / NW; ++ii) {
                const int i = NW * ii + wave;
                const int L = 64 * i + lane;
                const int r = L / CPR, pc = L % CPR;
                const unsigned off = (unsigned)(r * H + 8 * (pc ^ (r & 15))) * 2u;
                __builtin_amdgcn_global_load_lds(base + off, (__attribute__((address_space(3))) void *)(wbuf + 512 * i),
                                                 16, 0, 0);
            }
            return;
        }
#pragma unroll
        for (int ii = 0; ii < NI / NW; ++ii) {
            const int i = NW * ii + wave;
            const int L = 64 * i + lane;
            const int r = L / CPR, pc = L % CPR;
            const int v = min(32 * c + r, V - 1);
            const unsigned short *g = j.W + (int64_t)v * H + 8 * (pc ^ (r & 15));
            __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void *)(wbuf + 512 * i), 16, 0, 0);
        }
    }

    // one 32x32 output tile: D[vocab][row] = sum_k W[vocab][k] h[row][k]; A fragments stream from LDS
    // through a 4-deep register ring so no MFMA waits on a ds_read it has just issued. The swizzled piece of
    // k-step ks = 8m + k' is 16m + ((2k' + half) ^ (r & 15)): 8 base addresses, m in the immediate offset.
    template <int RING = 4>
    __device__ static __forceinline__ f32x16 mma(const unsigned short *wbuf, const bf16x8 (&bfr)[KS], int lane) {
        const int r = lane & 31, half = lane >> 5;
        const unsigned short *row = wbuf + r * H;
        const unsigned short *base[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) base[k] = row + 8 * ((2 * k + half) ^ (r & 15));
        auto rd = [&](int ks) { return *reinterpret_cast<const bf16x8 *>(base[ks & 7] + 128 * (ks >> 3)); };
        constexpr int D = KS < RING ? KS : RING;
        bf16x8 a[D];
#pragma unroll
        for (int d = 0; d < D; ++d) a[d] = rd(d);
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks % D], bfr[ks], acc, 0, 0, 0);
            if (ks + D < KS) a[ks % D] = rd(ks + D);
        }
        return acc;
    }
};

// The same W chunk as four 16x16 output tiles per wave (v_mfma_f32_16x16x32_bf16: at equal cycles per FLOP the
// 16x16 shape holds a higher clock than 32x32 on random operands, MI355X_MICROARCH.md 'DVFS give-back' item 7).
// A wave's 32 rows are two row tiles rt (rows 16 rt + (l & 15)); lane l holds k = 32 kk + 8 (l >> 4) + [0, 8) of
// both rows (B), and of W row 16 vt + (l & 15) (A: one ds_read_b128 feeds the MFMAs of both row tiles). Output
// d[vt][rt][r] = z(row 16 rt + (l & 15), vocab 32 c + 16 vt + 4 (l >> 4) + r).
template <int KS>
struct WTile16 {
    static constexpr int H = 16 * KS;
    static constexpr int K32 = KS / 2;  // MFMA k-steps
    struct Acc {
        f4 d[2][2];
    };

    // piece 4 kk + g of row 16 vt + c16 sits at (4 kk + g) ^ c16 (the WTile swizzle, c16 = row & 15): with
    // kk = 4 m + kk', that is 16 m + ((4 kk' + g) ^ c16): four base addresses, m and vt in the immediate offset
    template <int RING = 4>
    __device__ static __forceinline__ Acc mma(const unsigned short *wbuf, const bf16x8 (&bfr)[2][K32], int lane) {
        const int c16 = lane & 15, g = lane >> 4;
        const unsigned short *row = wbuf + c16 * H;
        const unsigned short *base[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) base[k] = row + 8 * ((4 * k + g) ^ c16);
        constexpr int NR = 2 * K32;  // A fragments per chunk, in (kk, vt) order
        auto rd = [&](int n) {
            const int kk = n >> 1, vt = n & 1;
            return *reinterpret_cast<const bf16x8 *>(base[kk & 3] + 128 * (kk >> 2) + 16 * H * vt);
        };
        constexpr int D = NR < RING ? NR : RING;
        bf16x8 a[D];
#pragma unroll
        for (int d = 0; d < D; ++d) a[d] = rd(d);
        Acc acc;
#pragma unroll
        for (int vt = 0; vt < 2; ++vt)
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) acc.d[vt][rt] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int n = 0; n < NR; ++n) {
            const int kk = n >> 1, vt = n & 1;
            acc.d[vt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[n % D], bfr[0][kk], acc.d[vt][0], 0, 0, 0);
            acc.d[vt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[n % D], bfr[1][kk], acc.d[vt][1], 0, 0, 0);
            if (n + D < NR) a[n % D] = rd(n + D);
        }
        return acc;
    }
};

__device__ __forceinline__ void wait_dma() { wait_vmcnt0(); }

// wait until at most N vector-memory operations of this wave are outstanding (in-order completion): the
// DMA of the chunk after next stays in flight across the barrier
template <int N>
__device__ __forceinline__ void wait_dma_leave() {
    static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
    __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}

// index of the accumulator register holding vocabulary offset jj (0..31) of a chunk, or -1 if the other lane
// half holds it
__device__ __forceinline__ int acc_reg_of(int jj, int half) {
    return (((jj >> 2) & 1) == half) ? ((jj & 3) + 4 * (jj >> 3)) : -1;
}

// vocabulary entry v lies in chunk c (wave-uniform for the blank: one chunk of a row holds it). Spelled on v - 32 c,
// as the backward always had it: v >= 32 c && v < 32 c + 32 is another test to the compiler (signed overflow) and
// changes the backward's code; the forward's drop_blank keeps that other spelling for the same reason.
__device__ __forceinline__ bool in_chunk(int v, int c) { return v - 32 * c >= 0 && v - 32 * c < 32; }

// this lane's accumulator register of the blank logit in chunk c, -1 where another chunk or the other lane half holds it
__device__ __forceinline__ int blank_reg(int blank, int c, int half) {
    return in_chunk(blank, c) ? acc_reg_of(blank - 32 * c, half) : -1;
}

// x[i] for a per-lane runtime i in [0, 16): a 4-level tree of bit selects (v_bfi_b32 on the bit masks of i;
// plain ternaries over arrays get rewritten into a scratch-indexed load)
__device__ __forceinline__ unsigned bsel(unsigned m, float a, float b) {  // m ? b : a, m all-ones or zero
    return (__float_as_uint(a) & ~m) | (__float_as_uint(b) & m);
}
__device__ __forceinline__ float tree_pick(const f2 (&x)[8], int i) {
    const unsigned m0 = 0u - (unsigned)(i & 1), m1 = 0u - (unsigned)((i >> 1) & 1);
    const unsigned m2 = 0u - (unsigned)((i >> 2) & 1), m3 = 0u - (unsigned)((i >> 3) & 1);
    const float a0 = __uint_as_float(bsel(m0, x[0].x, x[0].y)), a1 = __uint_as_float(bsel(m0, x[1].x, x[1].y));
    const float a2 = __uint_as_float(bsel(m0, x[2].x, x[2].y)), a3 = __uint_as_float(bsel(m0, x[3].x, x[3].y));
    const float a4 = __uint_as_float(bsel(m0, x[4].x, x[4].y)), a5 = __uint_as_float(bsel(m0, x[5].x, x[5].y));
    const float a6 = __uint_as_float(bsel(m0, x[6].x, x[6].y)), a7 = __uint_as_float(bsel(m0, x[7].x, x[7].y));
    const float b0 = __uint_as_float(bsel(m1, a0, a1)), b1 = __uint_as_float(bsel(m1, a2, a3));
    const float b2 = __uint_as_float(bsel(m1, a4, a5)), b3 = __uint_as_float(bsel(m1, a6, a7));
    const float c0 = __uint_as_float(bsel(m2, b0, b1)), c1 = __uint_as_float(bsel(m2, b2, b3));
    return __uint_as_float(bsel(m3, c0, c1));
}

// z = acc + bias as 8 packed pairs (pair k = registers 2k, 2k+1: vocabulary 32c + (2k&3) + 8(k>>1) + 4 half + {0,1});
// entries past V come out -inf through the padded bias
__device__ __forceinline__ void logits2(const f32x16 &acc, const float *bias_lds, int c, int half, f2 (&z)[8]) {
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        const f4 bv = *reinterpret_cast<const f4 *>(bias_lds + 32 * c + 8 * q4 + 4 * half);
        z[2 * q4] = add2((f2){acc[4 * q4], acc[4 * q4 + 1]}, (f2){bv.x, bv.y});
        z[2 * q4 + 1] = add2((f2){acc[4 * q4 + 2], acc[4 * q4 + 3]}, (f2){bv.z, bv.w});
    }
}

__device__ __forceinline__ float max3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// The factorised blank (HAT): register r of this lane's 16 becomes -inf (r = -1: none). Sixteen selects on the
// registers themselves (compile-time indices; an indexed array would go through scratch), run in the blank's chunk only.
__device__ __forceinline__ void drop_reg(f2 (&x)[8], int r) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        x[k].x = (2 * k == r) ? NEG_INF_F : x[k].x;
        x[k].y = (2 * k + 1 == r) ? NEG_INF_F : x[k].y;
    }
}

// Chunk loop: a workgroup of NW waves (NW = 8: two waves per SIMD, 256 rows) shares each W chunk; NB LDS buffers
// keep NB - 1 chunk DMAs in flight; one raw s_barrier per chunk. `S` = vector stores the epilogue issues per chunk
// on every wave (0 forward, 4 backward; -1 = unknown): the wait before chunk c leaves the later DMAs and the
// stores of the epilogues issued after chunk c's DMA in flight (vector memory completes in issue order).
// (Staggering the two waves of a SIMD by one epilogue, and three buffers, both measured slower: registers.)
// TRACE: stamp chunk 0 into the development build's forward timeline (the forward only: the backward kernels share
// this loop and would overwrite the same slots).
template <int KS, int NB, int NW, bool TRACE = false, class Mma, class Epi>
__device__ __forceinline__ void chunk_loop_with(const JointArgs &j, int V, unsigned short *wsh, int S, Mma &&mma,
                                                Epi &&epi) {
    using WT = WTile<KS>;
    constexpr int NPW = WT::NI / NW;  // DMA instructions per wave per chunk
    const int nch = (V + 31) / 32;
#pragma unroll
    for (int c = 0; c < NB - 1; ++c)
        if (c < nch) WT::template stage<NW>(j, V, c, wsh + c * WT::ELEMS);
    for (int c = 0; c < nch; ++c) {
        // chunk c in LDS for every wave
        if (c + NB - 2 < nch && S >= 0) {
            const int older = min(c, NB - 1);  // epilogues issued after chunk c's DMA
            if (S == 0 || older == 0) wait_dma_leave<(NB - 2) * NPW>();
            else if (older == 1) wait_dma_leave<(NB - 2) * NPW + 4>();
            else wait_dma_leave<(NB - 2) * NPW + 8>();  // NB == 3
        } else {
            wait_dma();
        }
        if (TRACE && c == 0) JOINT_MARK(5);
        __builtin_amdgcn_s_barrier();
        if (TRACE && c == 0) JOINT_MARK(6);
        if (c + NB - 1 < nch) WT::template stage<NW>(j, V, c + NB - 1, wsh + ((c + NB - 1) % NB) * WT::ELEMS);
        const auto acc = mma(wsh + (c % NB) * WT::ELEMS);
        if (TRACE && c == 0) JOINT_MARK(7);
        epi(acc, c);
    }
}

template <int KS, int NB, int NW, int RG, bool TRACE = false, class Epi>
__device__ __forceinline__ void chunk_loop(const JointArgs &j, int V, unsigned short *wsh, const bf16x8 (&bfr)[KS],
                                           int lane, int S, Epi &&epi) {
    chunk_loop_with<KS, NB, NW, TRACE>(j, V, wsh, S,
                                [&](const unsigned short *wb) { return WTile<KS>::template mma<RG>(wb, bfr, lane); },
                                epi);
}

// LDS: NB W tiles, then the bias padded to whole chunks
template <int KS, int NB>
__device__ __forceinline__ float *load_bias(const JointArgs &j, int V, unsigned short *wsh, bool scaled = false) {
    float *bl = reinterpret_cast<float *>(wsh + NB * WTile<KS>::ELEMS);
    const int nb = vpad(V);
    // past V: -inf, so z = acc + bias masks the tail chunk without a compare (the clamped W rows are finite);
    // scaled (the forward): a second row, bias * log2 e, right after it
    for (int v = threadIdx.x; v < nb; v += blockDim.x) {
        const float b = v < V ? (j.bias ? j.bias[v] : 0.0f) : NEG_INF_F;
        bl[v] = b;
        if (scaled) bl[nb + v] = b * kLog2e;
    }
    return bl;
}

// x[i] for a per-lane i in [0, 8): a 3-level select tree (v_cndmask; never an indexed register array)
__device__ __forceinline__ float pick8(const float (&x)[8], int i) {
    const bool b0 = i & 1, b1 = i & 2, b2 = i & 4;
    const float a0 = b0 ? x[1] : x[0], a1 = b0 ? x[3] : x[2], a2 = b0 ? x[5] : x[4], a3 = b0 ? x[7] : x[6];
    const float c0 = b1 ? a1 : a0, c1 = b1 ? a3 : a2;
    return b2 ? c1 : c0;
}

// vocabulary offset jj (0..31) of a chunk: held by lane group (jj >> 2) & 3 at index 4 (jj >> 4) + (jj & 3)
__device__ __forceinline__ int pick8_index(int jj) { return 4 * (jj >> 4) + (jj & 3); }

// z = acc + bias for row tile rt: x[4 vt + r] = vocabulary 32 c + 16 vt + 4 g + r (past V: -inf through the bias)
template <int KS>
__device__ __forceinline__ void logits8(const typename WTile16<KS>::Acc &acc, const f4 (&bv)[2], int rt,
                                        float (&x)[8]) {
#pragma unroll
    for (int vt = 0; vt < 2; ++vt)
#pragma unroll
        for (int r = 0; r < 4; ++r) x[4 * vt + r] = acc.d[vt][rt][r] + bv[vt][r];
}

}  // namespace mrnnt
