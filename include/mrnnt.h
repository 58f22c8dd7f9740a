/* mrnnt.h -- flat, pure-C ABI of libmonotonic_rnnt_amd.so (plain pointers and sizes only).
 *
 * This is the boundary every binding calls (the Python autograd op via ctypes, the C++ classes in
 * gpu_rnnt.h / rnnt_entrypoint.h, and any cgo/JNI/N-API stub: INTEGRATION.md). It replaces the
 * reference's pybind entry points (reference pytorch_binding/monotonic_rnnt.cu:81-152) and the
 * GpuRNNTComputer they construct (reference include/gpu_rnnt.h:27-235), split so an autograd
 * Function can run the loss in forward and the logit gradient (with dL/dcost fused) in backward.
 *
 * Data layout (same contract as the reference, monotonic_rnnt_op.py:133-140):
 *   acts    [N, V], N = sum_b T_b (S_b+1); utterance b contiguous, then t-major, then s ("packed").
 *           Extension (acts_layout): padded [B, pad_T, pad_S1, V] with (b, t, s) at row
 *           (b*pad_T + t)*pad_S1 + s -- the joint network's natural output, no packing copy.
 *           Element type fp32 (reference), or bf16 / fp16 (acts_dtype); grads use the same type and
 *           layout. The arithmetic is fp32/fp64 in registers whatever the element type.
 *   labels  [B, label_stride] int32, label of (b, s) at labels[b*label_stride + s]
 *   T, S    [B] int32 input / label lengths (device copies for the kernels, host copies to plan)
 *   alignment (optional) [B, align_stride] int32, frames equal to align_blank are blanks
 * All device pointers are HIP device memory; nothing is allocated inside the calls.
 */
#ifndef MONOTONIC_RNNT_MRNNT_H
#define MONOTONIC_RNNT_MRNNT_H

#include <stddef.h>
#include <stdint.h>

#include "options.h"
#include "status.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MRNNT_VERSION 13

/* acts / grads element types */
#define MRNNT_F32 0
#define MRNNT_BF16 1
#define MRNNT_F16 2

typedef struct mrnnt_problem {
    int B;                   /* utterances */
    int V;                   /* alphabet size including blank */
    int blank;               /* blank label index */
    int max_shift;           /* alignment restriction k (ignored when alignment == NULL) */
    const int *T_host;       /* host [B] */
    const int *S_host;       /* host [B] */
    const int *T_dev;        /* device [B] (same values) */
    const int *S_dev;        /* device [B] */
    const void *acts;        /* device [N, V] packed, or [B, pad_T, pad_S1, V] padded; acts_dtype elements */
    const int *labels;       /* device [B, label_stride] */
    int64_t label_stride;
    const int *alignment;    /* device [B, align_stride] or NULL */
    int64_t align_stride;
    int align_blank;         /* value marking blank frames in `alignment` */
    int64_t num_rows;        /* rows of acts as the caller sized it (checked; < 0 skips the check): packed
                                sum_b T_b (S_b+1), padded B*pad_T*pad_S1 */
    /* --- version 2 --- (zero-initialised = the reference contract: packed fp32) */
    int acts_dtype;          /* MRNNT_F32 / MRNNT_BF16 / MRNNT_F16 */
    int64_t pad_T;           /* padded layout: frames per utterance slot (>= max T_b) */
    int64_t pad_S1;          /* padded layout: label positions per frame (>= max S_b + 1); 0 = packed */
    /* --- version 4 --- */
    const void *lattice;     /* optional: device copy of mrnnt_lattice_host's output for these lengths. The lattice
                                offsets then come from it and mrnnt_forward launches no setup kernel (a caller that
                                repeats shapes uploads it once); NULL = built on the device in every forward. The
                                workspace then holds no offsets of its own: pass the same lattice to every later
                                call on that workspace (mrnnt_backward, mrnnt_read_*, mrnnt_grad_live_rows), and
                                only a lattice built from these lengths (it is not checked against them) */
    /* --- version 6 --- */
    int grad_scale_broadcast; /* 1: grad_scale[0] scales every utterance (a stride-0 upstream gradient, e.g. the
                                backward of costs.sum(): no copy into a [B] vector); 0: grad_scale[b] */
    /* --- version 7 --- */
    int lengths_on_device;   /* 1: the lengths exist only on the device (T_dev / S_dev; T_host / S_host may be NULL),
                                as the reference's GPU binding requires (monotonic_rnnt.cu:85-88). The launch is then
                                planned from bounds the host knows without reading them back -- num_rows (required:
                                the packed rows, or B*pad_T*pad_S1 padded) and label_stride (>= every S_b) -- and the
                                lattice offsets are built and the lengths validated on the device (T_b > 0, S_b >= 0,
                                T_b >= S_b, S_b <= label_stride, packed rows == num_rows, padded / alignment strides).
                                No host synchronisation; capturable in a HIP graph. lattice must be NULL. A length set
                                that fails validation makes every cost and gradient of the call NaN (nothing outside
                                the caller's buffers is touched) and raises *status_host. */
    int *status_host;        /* optional, with lengths_on_device: a host word from mrnnt_status_word(); the device
                                stores RNNT_STATUS_INVALID_VALUE into it when validation fails (never clears it) */
} mrnnt_problem;

/* A process-wide host-mapped int (initially 0) the device can store into without a copy: pass it as
 * mrnnt_problem.status_host and poll it from the host at leisure (reset it to 0 yourself). */
int *mrnnt_status_word(void);

/* Validate lengths (reference semantics: B > 0, V > 0, T_b > 0, S_b >= 0, T_b >= S_b) and return the
 * device workspace bytes needed by mrnnt_forward / mrnnt_backward for this problem. Host-only. */
RNNTStatus mrnnt_workspace_size(const mrnnt_problem *p, size_t *bytes);

/* Lattice offsets of the problem's lengths, computed on the host from T_host / S_host: int64 row_off[B+1]
 * (first lattice row of each utterance), int64 col_off[B+1] (first column), int32 col_b[sum_b T_b] (utterance
 * of each column). mrnnt_lattice_bytes gives the size; mrnnt_lattice_host fills `host` (>= that many bytes).
 * Upload it to device memory and pass it as mrnnt_problem.lattice. Host-only. */
RNNTStatus mrnnt_lattice_bytes(const mrnnt_problem *p, size_t *bytes);
RNNTStatus mrnnt_lattice_host(const mrnnt_problem *p, void *host, size_t bytes);

/* Forward: log-softmax row reduce + alpha (and, if with_beta, beta) recursion.
 * Writes costs_dev[b] = -log p(labels_b | acts_b) (device fp32, may be NULL) and keeps the per-row
 * state needed by mrnnt_backward in `workspace`. Asynchronous on `stream`. */
RNNTStatus mrnnt_forward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes, float *costs_dev,
                         int with_beta, hipStream_t stream);

/* Backward: grads[r, v] = grad_scale[b(r)] * dcost_b / dacts[r, v] for every row (out-of-band rows
 * are written with 0 * grad_scale, padding rows of the padded layout with 0; no pre-zeroing needed).
 * grads has the layout and element type of acts. grad_scale (device fp32 [B], or [1] with
 * grad_scale_broadcast) may be NULL (= 1).
 * Requires a preceding mrnnt_forward(with_beta=1) on the same workspace and inputs. */
RNNTStatus mrnnt_backward(const mrnnt_problem *p, const void *workspace, const float *grad_scale, void *grads,
                          hipStream_t stream);

/* (an addition to version 13: MRNNT_VERSION and both structs are unchanged) mrnnt_backward into a buffer whose
 * contents the caller can vouch for, so that rows which already hold the zero they would get are not stored again.
 * row_state: device memory, one byte per row of grads (rows of p->V elements of the acts type, in the layout of
 * acts), row_state_len of them. On entry the caller vouches, per row:
 *     0  unknown        1  every element of the row is +0.0        2  every element of the row is -0.0
 * In stream order on return grads holds, bit for bit, what mrnnt_backward would have written; row_state describes
 * the new contents of every row the call covers (0 for a row with a gradient or NaN, 1 / 2 for a row of +0 / -0;
 * all 0 when device lengths failed validation and grads is NaN); bytes past the rows the call covers are not touched.
 * A state byte that claims a zero the row does not hold gives a wrong gradient: whoever writes grads between two
 * calls must reset the bytes of the rows written (all 0 is always safe). grads must not alias acts.
 * row_state == NULL is exactly mrnnt_backward. row_state_len smaller than the rows covered (num_rows; padded layout:
 * B * pad_T * pad_S1) gives RNNT_STATUS_INVALID_VALUE before any device call. Rows are skipped by the vectorised
 * default kernel; the other gradient kernels (V or a pointer not 16-byte aligned; streamed rows of < 96 vectors)
 * write every row and leave the covered state 0. */
RNNTStatus mrnnt_backward_tracked(const mrnnt_problem *p, const void *workspace, const float *grad_scale, void *grads,
                                  unsigned char *row_state, int64_t row_state_len, hipStream_t stream);

/* forward(with_beta = grads != NULL) followed by backward. */
RNNTStatus mrnnt_cost_and_grad(const mrnnt_problem *p, void *workspace, size_t workspace_bytes, float *costs_dev,
                               void *grads, const float *grad_scale, hipStream_t stream);

/* (version 13) Best path (Viterbi alignment): for every utterance the single most probable monotonic path through
 * its T_b x (S_b+1) lattice, with the transitions and the band of mrnnt_forward (the alignment band too when
 * p->alignment restricts the call):
 *     v(t, s) = max(v(t-1, s) + lpb(t, s), v(t-1, s-1) + lpe(t, s-1)),   v(-1, s) = [s == 0 ? 0 : -inf]
 * in fp64. Tie rule (part of the contract, the same on both devices): the label arc is taken only when it is
 * STRICTLY greater than the blank arc; on a tie the frame emits blank.
 *   alignment_out_dev[b*out_stride + t], t < T_b: labels[b, s] when frame t emits label s, p->blank when it emits
 *       blank -- the format mrnnt_problem.alignment consumes with align_blank == blank; T_b <= t < out_stride: p->blank.
 *   costs_dev[b] = -v(T_b-1, S_b) (fp32; may be NULL): the negative log-probability of that one path.
 * Sentinels: no finite path (masked -inf logits, or a restricting band no path fits): cost +inf and the whole row
 * (all out_stride entries) -1. A NaN or +inf logit inside the utterance's band: cost NaN and the row -1; the other
 * utterances are unaffected. Device-resident lengths that fail validation: every cost NaN, every row -1 and
 * *status_host raised, as mrnnt_forward does.
 * out_stride >= max_b T_b (host lengths: checked here; lengths_on_device: T_b <= out_stride joins the device
 * validation). Takes everything mrnnt_forward's log-softmax pass takes (bf16 / fp16 acts, the padded layout, a
 * restricting alignment with max_shift, device-resident lengths: no host read, capturable). p->alignment and
 * alignment_out_dev may be the same buffer (the band is built from the input before the output is written).
 * No new workspace: mrnnt_workspace_size is the size query (the back-pointers, one bit per cell, use the alpha array
 * of the workspace, so the call overwrites the state of an earlier mrnnt_forward). Asynchronous on `stream`. */
RNNTStatus mrnnt_align(const mrnnt_problem *p, void *workspace, size_t workspace_bytes, int *alignment_out_dev,
                       int64_t out_stride, float *costs_dev, hipStream_t stream);

/* Arc posteriors of the lattice, read out of the workspace after mrnnt_forward(with_beta = 1) on the same workspace
 * and inputs (an addition to version 13: MRNNT_VERSION and every struct are unchanged, so callers that may meet an
 * older build of version 13 probe for the symbols mrnnt_posteriors / mrnnt_cpu_posteriors). With alpha(t, s) the state
 * after frame t (alpha(-1, s) = [s == 0 ? 0 : -inf]), beta(t, s) the state before frame t (beta(T, s) = [s == S ? 0 :
 * -inf]) and ll = alpha(T-1, S), for lattice row (b, t, s):
 *     blank_post(t, s) = exp(alpha(t-1, s) + lpb(t, s) + beta(t+1, s)   - ll)   P(frame t takes the blank arc out of (t, s))
 *     label_post(t, s) = exp(alpha(t-1, s) + lpe(t, s) + beta(t+1, s+1) - ll)   (s < S_b; 0 at s = S_b)
 *     emit(b, t)       = sum_s label_post(t, s)                                 P(frame t emits a label)
 *     label_time(b, s) = sum_t t * label_post(t, s)   (s < S_b)                 expected frame at which label s is emitted
 * formed in fp64 from the fp64 state and stored as fp32 -- the two per-row coefficients of the logit gradient. With a
 * restricting alignment they are the posteriors of the restricted distribution. For every frame sum_s (blank_post +
 * label_post) = 1, for every label sum_t label_post = 1, and sum_t emit = S_b.
 *   blank_post_dev / label_post_dev: one value per row of acts, in acts' row layout like grads (packed [N]; padded
 *       [B, pad_T, pad_S1], padding rows 0), so the host can size them even with lengths_on_device.
 *   emit_dev [B, emit_stride]: 0 for t >= T_b.      label_time_dev [B, time_stride]: -1 for s >= S_b.
 *   Any output may be NULL (its work is skipped).
 * Unreachable rows (alpha(t-1, s) or beta(t, s) = -inf: outside the monotonic band or a restricting alignment band,
 * masked logits) are exactly 0. An utterance whose ll is not finite (no path: cost +inf; a NaN / +inf logit in its band)
 * has every per-row value, emit(b, t < T_b) and label_time(b, s < S_b) NaN; the other utterances are unaffected.
 * Strides: host lengths -- emit_stride >= max T_b and time_stride >= max S_b are checked here, with the NULL
 * workspace, before any device call (RNNT_STATUS_INVALID_VALUE). lengths_on_device -- nothing is written past a
 * stride: an utterance with T_b > emit_stride (S_b > time_stride) gets its emit (label_time) row NaN and *status_host
 * is raised; lengths that failed the forward's validation make every output element, as the host sized it, NaN.
 * Every sum has a fixed order with fp64 accumulation (bitwise reproducible). Reads the workspace only (not acts, not
 * labels); no new workspace and no size query; no host read, capturable; asynchronous on `stream`. Its launch counts
 * under [2] of mrnnt_profile_read. */
RNNTStatus mrnnt_posteriors(const mrnnt_problem *p, const void *workspace, float *blank_post_dev, float *label_post_dev,
                            float *emit_dev, int64_t emit_stride, float *label_time_dev, int64_t time_stride,
                            hipStream_t stream);

/* Whole alignments drawn from the path posterior p(path | labels, acts), read out of the workspace after
 * mrnnt_forward(with_beta = 1) on the same workspace and inputs (an addition to version 13: MRNNT_VERSION and every
 * struct are unchanged, so callers that may meet an older build of version 13 probe for the symbols mrnnt_sample /
 * mrnnt_cpu_sample / mrnnt_joint_sample). The third read-out of the lattice next to mrnnt_align (max) and
 * mrnnt_posteriors (sum). A walker starts at s = 0 before frame 0 and goes forward in time. On row (t, s), with
 * beta(T, s) = [s == S ? 0 : -inf]:
 *     x = lpb(t, s) + beta(t+1, s)       the blank arc; -inf when it would leave the monotonic band (T-1-t < S-s)
 *     y = lpe(t, s) + beta(t+1, s+1)     the label arc; -inf at s = S
 *     p_label = 1 / (1 + exp(x - y))     fp64; y = -inf: 0, else x = -inf: 1; the two arcs sum to exactly 1
 *     frame t emits labels[b, s] (and s += 1) iff u(b, k, t) < p_label, else blank (a NaN p_label emits blank)
 * With a restricting alignment the draws come from the restricted distribution (its band is -inf in the state).
 * Random numbers (the contract, identical on both devices): Philox4x32-10 with key (seed low 32 bits, seed high 32
 * bits) and counter (t >> 2, first_sample + k, b, 0x4D524E54); frame t uses output word t & 3 as
 * u = (word + 0.5) * 2^-32. So sample (b, k) depends on (seed, b, first_sample + k, t) and the state alone -- not on
 * num_samples, the other utterances or the launch: results are bitwise reproducible, and a call with 8 samples
 * returns the first 8 of a call with 64.
 *   alignments_dev[(b*num_samples + k)*out_stride + t], t < T_b: the label frame t emits or p->blank -- the format
 *       mrnnt_problem.alignment consumes with align_blank == blank; T_b <= t < out_stride: p->blank.
 *   path_costs_dev[b*num_samples + k] (may be NULL): fp32 of -sum_t lp(chosen arc), summed in fp64 in frame order:
 *       the negative log-probability of that path under the model.
 * Sentinels, as mrnnt_align: an utterance whose log-likelihood is not finite has all its num_samples rows -1 and its
 * path costs +inf (no path) or NaN (a NaN / +inf logit in its band); the other utterances are bit-identical to a call
 * without it. Device-resident lengths that failed the forward's validation: every row -1 and every path cost NaN.
 * lengths_on_device and T_b > out_stride: that utterance's rows -1, its path costs NaN, nothing written past the
 * stride, *status_host raised.
 * Checked on the host before any device call (RNNT_STATUS_INVALID_VALUE): num_samples >= 1; first_sample >= 0 and
 * first_sample + num_samples <= 2^32; alignments_dev != NULL; out_stride >= max T_b (host lengths).
 * Reads the workspace, labels and the lengths (never acts); no new workspace and no size query; no host read,
 * capturable; asynchronous on `stream`. Its launch counts under [2] of mrnnt_profile_read. */
RNNTStatus mrnnt_sample(const mrnnt_problem *p, const void *workspace, int num_samples, uint64_t seed,
                        int64_t first_sample, int *alignments_dev, int64_t out_stride, float *path_costs_dev,
                        hipStream_t stream);

/* Differentiable scores of GIVEN alignments (an addition to version 13: MRNNT_VERSION and every struct are unchanged,
 * so callers that may meet an older build of version 13 probe for the symbols mrnnt_path_forward / mrnnt_cpu_path_forward).
 * The read-outs above take paths out of the lattice (mrnnt_align the best one, mrnnt_sample draws); this pair scores
 * num_paths of them per utterance and returns the logit gradient of sum_{b,k} w[b, k] * path_costs[b, k] -- Viterbi
 * training, risk-weighted / MWER / REINFORCE objectives over sampled paths (signed weights), latency penalties -- in one
 * forward and ONE dense gradient pass whatever num_paths is.
 *   alignments_dev[(b*num_paths + k)*path_stride + t], t < T_b: p->blank, or the label frame t emits -- the format
 *       mrnnt_align / mrnnt_sample write. Entries at t >= T_b are not read.
 * Walk of row (b, k), from s = 0: at frame t an entry equal to p->blank takes the blank arc of row (t, s); an entry
 * equal to labels[b, s] with s < S_b takes the label arc, then s += 1; anything else (a wrong label, a negative value,
 * the -1 sentinel rows, a label at s = S_b) makes the row INVALID, and so does s != S_b after frame T_b - 1.
 * Forward: path_costs_dev[b*num_paths + k] (may be NULL) = fp32(-sum_t lp(arc_t)), lp = z[row, v] + den[row] as the
 *   loss forms it, summed in fp64 in a fixed order (bitwise reproducible). An invalid row costs +inf. A path through a
 *   -inf logit costs +inf; a NaN or +inf logit in a visited row gives NaN for the paths that visit it; the other paths
 *   and utterances are bit-identical to a call without it. The log-softmax reads only the rows between the lowest and
 *   the highest valid path of each frame (the hull), plus row (0, 0) of an utterance without a valid path.
 * Backward (after mrnnt_path_forward on the same workspace, problem and alignments): weights_dev[b*num_paths + k]
 *   (fp32, signed; NULL = 1) is the upstream gradient of path_costs. With Wb(r) / We(r) the sums of w[b, k] over the
 *   VALID paths that take the blank / label arc out of row r, accumulated in fp64 in ascending k, and Wocc = Wb + We,
 *       grads[r, v] = Wocc(r) softmax(z_r)[v] - [v == blank] Wb(r) - [v == label(s)] We(r).
 *   The weight of an invalid path is ignored. A row with Wb == 0 && We == 0 (unvisited, outside every path, an
 *   utterance without a valid path, all-zero weights) is stored as exact zeros and its acts are not read (a NaN logit
 *   there gives 0); Wb = -We != 0 is a live row with Wocc = 0. Padding rows of the padded layout are 0. grads has the
 *   layout and element type of acts; no pre-zeroing; every gradient is bitwise reproducible.
 * Takes everything mrnnt_forward's log-softmax pass takes (bf16 / fp16 acts, the padded layout, device-resident
 * lengths: no host read, capturable; T_b <= path_stride then joins the device validation, and a failed validation
 * makes every path cost and gradient NaN and raises *status_host, as the loss does) except a restricting alignment:
 * the band arrays of the workspace hold the hull.
 * Checked on the host before any device call, workspace included (RNNT_STATUS_INVALID_VALUE): p->alignment == NULL;
 * num_paths >= 1; alignments_dev != NULL; path_stride >= max T_b (host lengths).
 * Workspace: mrnnt_path_workspace_size(p, num_paths) bytes (>= mrnnt_workspace_size: the loss's arrays, the band
 * arrays and a few words per path); Wb / We use its alpha / beta arrays. Asynchronous on `stream`. The new launches
 * count under [2] of mrnnt_profile_read, the log-softmax under [1], the gradient under [3]. */
RNNTStatus mrnnt_path_workspace_size(const mrnnt_problem *p, int num_paths, size_t *bytes);
RNNTStatus mrnnt_path_forward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                              const int *alignments_dev, int num_paths, int64_t path_stride, float *path_costs_dev,
                              hipStream_t stream);
RNNTStatus mrnnt_path_backward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                               const int *alignments_dev, int num_paths, int64_t path_stride, const float *weights_dev,
                               void *grads, hipStream_t stream);
/* (an addition to version 13) mrnnt_path_backward with the row state of mrnnt_backward_tracked: the same contract,
 * the same bytes, so one buffer and one state can serve loss and path gradients in turn. */
RNNTStatus mrnnt_path_backward_tracked(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                       const int *alignments_dev, int num_paths, int64_t path_stride,
                                       const float *weights_dev, void *grads, unsigned char *row_state,
                                       int64_t row_state_len, hipStream_t stream);

/* Expected path costs with a gradient (an addition to version 13: MRNNT_VERSION and every struct are unchanged, so
 * callers that may meet an older build of version 13 probe for the symbols mrnnt_expect_forward /
 * mrnnt_cpu_expect_forward). For a cost that adds up over the arcs of a path -- emission time (expected latency), blank
 * count, a per-arc risk -- the expectation under p(path | labels, acts) and its logit gradient are exact lattice
 * quantities (the first-order expectation semiring): no sampling. Conventions as mrnnt_posteriors: alpha(t, s) after
 * frame t (alpha(-1, s) = [s == 0]), beta(t, s) before frame t (beta(T, s) = [s == S]), ll = alpha(T-1, S); row (t, s)
 * has a blank arc to (t+1, s) and, for s < S, a label arc to (t+1, s+1).
 *   blank_cost_dev / label_cost_dev: wb / we, one fp32 per row of acts in acts' row layout -- the layout of
 *       mrnnt_posteriors' blank_post / label_post: packed [N], or [B, pad_T, pad_S1]. Either may be NULL (all zeros).
 *       we at s = S_b and anything at padding rows is never used. f(path) = sum_t cost(arc_t).
 *   expected[b] = sum_path p(path) f(path) / sum_path p(path)      (= sum_rows blank_post wb + label_post we)
 *   A(t, s)  = [e^(alpha(t-1,s)+lpb(t,s)) (A(t-1,s)+wb(t,s)) + e^(alpha(t-1,s-1)+lpe(t,s-1)) (A(t-1,s-1)+we(t,s-1))] / e^alpha(t,s)
 *   Bk(t, s) = [e^(lpb(t,s)+beta(t+1,s)) (wb(t,s)+Bk(t+1,s)) + e^(lpe(t,s)+beta(t+1,s+1)) (we(t,s)+Bk(t+1,s+1))] / e^beta(t,s)
 *   A(-1, .) = 0, Bk(T, .) = 0, R = expected[b] = A(T-1, S) = Bk(0, 0)
 *   cb(t, s) = blank_post(t, s) (A(t-1, s) + wb(t, s) + Bk(t+1, s)   - R)
 *   ce(t, s) = label_post(t, s) (A(t-1, s) + we(t, s) + Bk(t+1, s+1) - R)        (0 at s = S)
 *   d expected / d z[r, v] = cb ([v == blank] - softmax(z_r)[v]) + ce ([v == label(s)] - softmax(z_r)[v])
 * A and Bk are convex combinations (signed costs are fine), fp64 state, 0 on cells no path reaches; the two weights of
 * a step sum to exactly 1. A single-path lattice (S = 0, S = T) has a zero gradient.
 * mrnnt_expect_forward: mrnnt_forward (costs_dev[b] = the loss, may be NULL; with_grad: with beta) and then ONE launch
 *   that carries A forward and -- with_grad -- Bk backward, concurrently; expected_dev[b] = fp32(R) (may be NULL).
 * mrnnt_expect_backward (after mrnnt_expect_forward(with_grad = 1) on the same workspace, problem and costs): the logit
 *   gradient of sum_b g_e[b] expected[b] + g_c[b] costs[b] in ONE dense pass (grad_expected_dev / grad_costs_dev: fp32
 *   [B], either may be NULL = 0 for that term):
 *       Wb = g_c blank_post - g_e cb,   We = g_c label_post - g_e ce
 *       grads[r, v] = (Wb + We) softmax(z_r)[v] - [v == blank] Wb - [v == label(s)] We.
 *   A row whose two fp32 coefficients are both zero (outside the band, unreachable, underflow) is stored as exact zeros
 *   without reading its acts. Padding rows of the padded layout are 0. grads has the layout and element type of acts.
 *   mrnnt_expect_backward_tracked: the same with the row state of mrnnt_backward_tracked (the same contract and bytes).
 * An utterance whose ll is not finite has expected[b] NaN and every one of its gradient rows NaN (as the loss for
 * ll = -inf); the other utterances are bit-identical to a call without it. Device-resident lengths that fail
 * validation give NaN everywhere and raise *status_host, as the loss does. The cost arrays are not differentiated
 * (their gradient is mrnnt_posteriors' blank_post / label_post). Every sum has a fixed order and no atomics: results
 * are bitwise reproducible and do not depend on the other utterances.
 * Takes everything mrnnt_forward takes: bf16 / fp16 acts, the padded layout, device-resident lengths (no host read,
 * capturable), and a restricting p->alignment -- the expectation is then under the restricted distribution.
 * Checked on the host before any device call (RNNT_STATUS_INVALID_VALUE): everything mrnnt_forward checks, a NULL or
 * too small workspace, NULL grads. Workspace: mrnnt_expect_workspace_size(p) bytes (>= mrnnt_workspace_size: the loss's
 * arrays, then A, Bk and R). Asynchronous on `stream`. The recursion launch counts under [2] of mrnnt_profile_read, the
 * gradient under [3]. */
RNNTStatus mrnnt_expect_workspace_size(const mrnnt_problem *p, size_t *bytes);
RNNTStatus mrnnt_expect_forward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                const float *blank_cost_dev, const float *label_cost_dev, float *expected_dev,
                                float *costs_dev, int with_grad, hipStream_t stream);
RNNTStatus mrnnt_expect_backward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                 const float *blank_cost_dev, const float *label_cost_dev,
                                 const float *grad_expected_dev, const float *grad_costs_dev, void *grads,
                                 hipStream_t stream);
RNNTStatus mrnnt_expect_backward_tracked(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                         const float *blank_cost_dev, const float *label_cost_dev,
                                         const float *grad_expected_dev, const float *grad_costs_dev, void *grads,
                                         unsigned char *row_state, int64_t row_state_len, hipStream_t stream);

/* ---- factorised blank (the hybrid autoregressive transducer's output distribution; an addition to version 13:
 * MRNNT_VERSION and the structs are unchanged, callers probe for the symbols) ------------------------------------
 * The same lattice, band, alignment restriction, recursion and cost as mrnnt_forward, over another distribution per
 * row z: blank (index b = p->blank, anywhere in [0, V)) is a Bernoulli on its own logit and the labels are a softmax
 * over the other V - 1 logits,
 *     lp_blank = log sigmoid(z_b),    lp_label = log sigmoid(-z_b) + z_l - LSE_{v != b} z_v.
 * With cb / ce the blank-arc / label-arc posteriors of a row (mrnnt_posteriors' blank_post / label_post), the gradient
 * mrnnt_hat_backward writes, times grad_scale, is
 *     g[b] = ce sigmoid(z_b) - cb sigmoid(-z_b),    g[v != b] = ce (softmax_{u != b}(z)[v] - [v == label(s)])
 * (at s = S_b: ce = 0, only g[b] is non-zero). A row whose ce and blank element are both zero in fp32 is stored as
 * exact zeros without reading its acts. LSE_{v != b} keeps z_b out of the max and the sum (nothing is subtracted from a
 * whole-row sum), each sigmoid is formed by itself in its stable form: a blank logit of +-100 over N(0,1) labels loses
 * nothing. The passes move exactly the bytes of mrnnt_forward / mrnnt_backward.
 * Non-finite logits keep the loss's meaning: a -inf label logit or z_b = -inf is "no such arc" (+inf cost when every
 * path needs it); a NaN or +inf logit in an utterance's band, z_b = +inf included, makes that utterance's cost NaN;
 * the other utterances are bit-identical either way. A label equal to blank is no label arc. A -inf on any other
 * logit only removes that entry's mass; a row whose non-blank logits are all -inf (every row at V = 1) has no label
 * arc (-inf, not NaN) and an unchanged blank arc, and den' = +inf there.
 * mrnnt_hat_forward / mrnnt_hat_backward / mrnnt_hat_backward_tracked / mrnnt_hat_align take the arguments, the host
 * checks, the layouts, element types, device-resident lengths, alignment restriction, row state and profile slots of
 * mrnnt_forward / mrnnt_backward / mrnnt_backward_tracked / mrnnt_align, and the workspace is mrnnt_workspace_size(p)
 * bytes. The forward never takes the single-launch (chase) form. mrnnt_posteriors and mrnnt_sample read only lp /
 * alpha / beta / ll and work unchanged on the workspace of mrnnt_hat_forward(with_beta = 1); mrnnt_backward on such a
 * workspace (or mrnnt_hat_backward after mrnnt_forward) is an error the library cannot detect. mrnnt_read_state's and
 * mrnnt_read_denoms' den is -LSE_{v != b} on the rows a factorised forward reduced.
 * mrnnt_hat_path_* / mrnnt_hat_expect_* (below) are the factorised forms of mrnnt_path_* / mrnnt_expect_* over stored
 * logits; the fused joint's path scores and expected costs have no factorised form yet. */
RNNTStatus mrnnt_hat_forward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes, float *costs_dev,
                             int with_beta, hipStream_t stream);
RNNTStatus mrnnt_hat_backward(const mrnnt_problem *p, const void *workspace, const float *grad_scale, void *grads,
                              hipStream_t stream);
RNNTStatus mrnnt_hat_backward_tracked(const mrnnt_problem *p, const void *workspace, const float *grad_scale,
                                      void *grads, unsigned char *row_state, int64_t row_state_len,
                                      hipStream_t stream);
RNNTStatus mrnnt_hat_align(const mrnnt_problem *p, void *workspace, size_t workspace_bytes, int *alignment_out_dev,
                           int64_t out_stride, float *costs_dev, hipStream_t stream);

/* Path scores and expected path costs under the factorised blank (an addition to version 13: MRNNT_VERSION and every
 * struct are unchanged, callers probe for the symbols mrnnt_hat_path_forward / mrnnt_hat_expect_forward and their
 * mrnnt_cpu_ twins). Both objectives are -sum_rows (Wb lpb + We lpe) with signed per-row arc weights -- path scores: Wb
 * / We the summed upstream weights of the valid paths that leave the row by its blank / label arc; expected costs:
 * Wb = g_c blank_post - g_e cb, We = g_c label_post - g_e ce exactly as mrnnt_expect_backward forms them -- and the
 * gradient through the factorised row, with den' = -LSE_{u != b} z_u, is
 *     g[b]      = We sigmoid(z_b) - Wb sigmoid(-z_b)
 *     g[v != b] = We (exp(z_v + den') - [v == label(s)]).
 * We is signed and may be exactly 0 while Wb is not (a row visited by blank arcs only): it multiplies the exponential,
 * it is not folded into the exponent. The blank element is formed once per row from lpb = log sigmoid(z_b), each
 * sigmoid by itself and the two products in fp64 before one rounding; it is never read off exp(z_b + den'), which
 * overflows once the blank dominates the row.
 * Zero rows: a row is stored as exact zeros without reading its acts where Wb == 0 && We == 0 (path scores: in fp64,
 * so Wb = -We != 0 stays live; expected costs: both fp32 coefficients). Rows outside the hull / band and dead rows are
 * stored as the softmax entry points store them: 0, or NaN for an utterance of mrnnt_hat_expect_* whose ll is not
 * finite. A row whose non-blank logits are all -inf (den' = +inf) has no label arc: its non-blank elements are exact
 * zeros and only g[b] survives. A NaN or +inf logit on a live row (z_b = +inf included) makes the whole row NaN.
 * Each function takes exactly the arguments, host checks, layouts, element types, device-resident lengths, row state,
 * workspace size (mrnnt_path_workspace_size / mrnnt_expect_workspace_size serve both) and profile slots of its twin
 * without _hat; the forwards run the factorised log-softmax (over the hull; mrnnt_hat_forward for the expectation,
 * never the chase launch), every other forward kernel is the twin's own: the walk, hull, score and coefficient kernels
 * and the expectation recursion read lp / alpha / beta / den, never a logit. costs_dev of mrnnt_hat_expect_forward is
 * mrnnt_hat_forward's, bit for bit. A softmax backward on a factorised forward's workspace (or the reverse) is an
 * error the library cannot detect. */
RNNTStatus mrnnt_hat_path_forward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                  const int *alignments_dev, int num_paths, int64_t path_stride, float *path_costs_dev,
                                  hipStream_t stream);
RNNTStatus mrnnt_hat_path_backward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                   const int *alignments_dev, int num_paths, int64_t path_stride,
                                   const float *weights_dev, void *grads, hipStream_t stream);
RNNTStatus mrnnt_hat_path_backward_tracked(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                           const int *alignments_dev, int num_paths, int64_t path_stride,
                                           const float *weights_dev, void *grads, unsigned char *row_state,
                                           int64_t row_state_len, hipStream_t stream);
RNNTStatus mrnnt_hat_expect_forward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                    const float *blank_cost_dev, const float *label_cost_dev, float *expected_dev,
                                    float *costs_dev, int with_grad, hipStream_t stream);
RNNTStatus mrnnt_hat_expect_backward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                     const float *blank_cost_dev, const float *label_cost_dev,
                                     const float *grad_expected_dev, const float *grad_costs_dev, void *grads,
                                     hipStream_t stream);
RNNTStatus mrnnt_hat_expect_backward_tracked(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                             const float *blank_cost_dev, const float *label_cost_dev,
                                             const float *grad_expected_dev, const float *grad_costs_dev, void *grads,
                                             unsigned char *row_state, int64_t row_state_len, hipStream_t stream);

/* Forward log-likelihoods from the workspace (device double [B]), for debugging/inspection:
 * ll_fwd = alpha(T-1, S), ll_bwd = beta(0, 0). Either may be NULL. Asynchronous on `stream`. */
RNNTStatus mrnnt_read_loglik(const mrnnt_problem *p, const void *workspace, double *ll_fwd_dev, double *ll_bwd_dev,
                             hipStream_t stream);

/* Per-row state of the last mrnnt_forward on this workspace, for inspection / parity tests: den[r] (fp32
 * log-softmax denominator -max - log sum exp(z - max) of the rows the forward reduced: the in-band or
 * alignment-window rows, 0 elsewhere), alpha[r] = alpha(t, s) and beta[r] = beta(t, s) (fp64, -inf outside the
 * band; beta only after with_beta = 1), all in the packed lattice row order r = sum_{b'<b} T_b'(S_b'+1) +
 * t (S_b+1) + s. Device buffers of N elements; any may be NULL. Asynchronous on `stream`. */
RNNTStatus mrnnt_read_state(const mrnnt_problem *p, const void *workspace, float *den_dev, double *alpha_dev,
                            double *beta_dev, hipStream_t stream);

/* Log-softmax denominator of EVERY lattice row, den[r] = -max_v z - log sum_v exp(z - max) in the packed row
 * order of mrnnt_read_state (the reference's denom_host(), gpu_workspace_manager.h:137-141, whose reduce covers
 * all rows): the rows the last mrnnt_forward reduced are copied from the workspace, the others (outside the band or
 * the alignment window, which the forward never reads) are reduced from acts here. den_dev: device fp32 [N].
 * Asynchronous on `stream`. */
RNNTStatus mrnnt_read_denoms(const mrnnt_problem *p, const void *workspace, float *den_dev, hipStream_t stream);

/* The alignment band of the problem in the reference's [B, ld] layout (gpu_workspace_manager.h:167-177,191-219):
 * min_dev[b*ld + t] / max_dev[b*ld + t] = the lowest / highest label position alpha(t, .) may take, for t < T_b;
 * 0 / S_b for t >= T_b and for every t without an alignment (the reference's initial values, :317-328). Builds the
 * band in `workspace` from p->alignment (device kernels, as mrnnt_forward does), so it needs no preceding
 * forward. ld >= max T_b; either output may be NULL. Asynchronous on `stream`. */
RNNTStatus mrnnt_read_band(const mrnnt_problem *p, void *workspace, int *min_dev, int *max_dev, int64_t ld,
                           hipStream_t stream);

/* Message describing the last non-success status returned on this thread. */
const char *mrnnt_last_error(void);

/* Number of in-band lattice rows whose acts the gradient kernel reads ("live" rows) for the problem of the
 * last mrnnt_forward(with_beta=1) on this workspace, written to *count_dev (device uint64). A row whose
 * occupancy exp(alpha(t-1,s) + beta(t,s) - ll) is below e^-110 has an exactly-zero fp32 gradient and is
 * stored without reading acts ("occ_skip" knob, on by default), and so is a row of mrnnt_backward whose every
 * fp32 exponential flushes to zero (occupancy below about e^-87.35 and both arc corrections 0: the same bits
 * either way). Inspection/bench only; asynchronous. */
RNNTStatus mrnnt_grad_live_rows(const mrnnt_problem *p, const void *workspace, unsigned long long *count_dev,
                                hipStream_t stream);

/* ---- host implementation (RNNT_CPU; reference cpu_rnnt.h / pytorch_binding cpu_monotonic_rnnt) --------
 * The same problem description with every pointer on the HOST: acts (fp32 only), labels, alignment,
 * T_host / S_host (T_dev / S_dev are ignored), workspace, costs, grads, grad_scale. Lengths, strides and
 * labels are validated (a label outside [0, V) is RNNT_STATUS_INVALID_VALUE). num_threads <= 0 uses the
 * OpenMP default. Results follow the GPU path's semantics (fp64 recursion, occupancy-exact zero rows). */
RNNTStatus mrnnt_cpu_workspace_size(const mrnnt_problem *p, size_t *bytes);

/* Log-softmax row reduce + alpha (and, if with_beta, beta) recursion; costs[b] = -log p (may be NULL). */
RNNTStatus mrnnt_cpu_forward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes, float *costs,
                             int with_beta, int num_threads);

/* grads[r, v] = grad_scale[b(r)] * dcost_b / dacts[r, v] for every row (grad_scale may be NULL = 1), after
 * mrnnt_cpu_forward(with_beta=1) on the same workspace and inputs. grads may be acts itself (in place). */
RNNTStatus mrnnt_cpu_backward(const mrnnt_problem *p, const void *workspace, const float *grad_scale, float *grads,
                              int num_threads);

/* mrnnt_read_state for the host implementation (host buffers). */
RNNTStatus mrnnt_cpu_read_state(const mrnnt_problem *p, const void *workspace, float *den, double *alpha,
                                double *beta);

/* (version 13) mrnnt_align for the host implementation: alignment_out [B, out_stride] and costs (may be NULL) on the
 * host, mrnnt_cpu_workspace_size bytes of workspace. Same tie rule and sentinels as mrnnt_align. */
RNNTStatus mrnnt_cpu_align(const mrnnt_problem *p, void *workspace, size_t workspace_bytes, int *alignment_out,
                           int64_t out_stride, float *costs, int num_threads);

/* mrnnt_posteriors for the host implementation, after mrnnt_cpu_forward(with_beta = 1) on the same workspace: host
 * buffers, the same values, rules and stride checks (sums in index order, fp64). */
RNNTStatus mrnnt_cpu_posteriors(const mrnnt_problem *p, const void *workspace, float *blank_post, float *label_post,
                                float *emit, int64_t emit_stride, float *label_time, int64_t time_stride,
                                int num_threads);

/* mrnnt_sample for the host implementation, after mrnnt_cpu_forward(with_beta = 1) on the same workspace: host
 * buffers, the same walk, random numbers, sentinels and checks (the same integer code and decision rule; a sample
 * can differ from the device's only where some frame's u lies within the two states' rounding of its p_label). */
RNNTStatus mrnnt_cpu_sample(const mrnnt_problem *p, const void *workspace, int num_samples, uint64_t seed,
                            int64_t first_sample, int *alignments, int64_t out_stride, float *path_costs,
                            int num_threads);

/* mrnnt_path_workspace_size / mrnnt_path_forward / mrnnt_path_backward for the host implementation: host buffers
 * (fp32 acts), the same walk, validity rule, sums (fp64, frame order / ascending k), exact zeros and host checks.
 * grads may be acts itself (in place), as in mrnnt_cpu_backward. */
RNNTStatus mrnnt_cpu_path_workspace_size(const mrnnt_problem *p, int num_paths, size_t *bytes);
RNNTStatus mrnnt_cpu_path_forward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes, const int *alignments,
                                  int num_paths, int64_t path_stride, float *path_costs, int num_threads);
RNNTStatus mrnnt_cpu_path_backward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes, const int *alignments,
                                   int num_paths, int64_t path_stride, const float *weights, float *grads,
                                   int num_threads);

/* mrnnt_expect_workspace_size / mrnnt_expect_forward / mrnnt_expect_backward for the host implementation: host buffers
 * (fp32 acts), the same formulas, masks, exact zeros, NaN rule and host checks, in fp64 with the library exp. */
RNNTStatus mrnnt_cpu_expect_workspace_size(const mrnnt_problem *p, size_t *bytes);
RNNTStatus mrnnt_cpu_expect_forward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                    const float *blank_cost, const float *label_cost, float *expected, float *costs,
                                    int with_grad, int num_threads);
RNNTStatus mrnnt_cpu_expect_backward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                     const float *blank_cost, const float *label_cost, const float *grad_expected,
                                     const float *grad_costs, float *grads, int num_threads);

/* mrnnt_hat_forward / mrnnt_hat_backward / mrnnt_hat_align for the host implementation: host buffers (fp32 acts),
 * mrnnt_cpu_workspace_size bytes of workspace, the same formulas, masking, dead-row rule and non-finite rules in fp64
 * with the library exp / log1p. mrnnt_cpu_posteriors and mrnnt_cpu_sample work unchanged after
 * mrnnt_cpu_hat_forward(with_beta = 1). grads may be acts itself (in place), as in mrnnt_cpu_backward. */
RNNTStatus mrnnt_cpu_hat_forward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes, float *costs,
                                 int with_beta, int num_threads);
RNNTStatus mrnnt_cpu_hat_backward(const mrnnt_problem *p, const void *workspace, const float *grad_scale, float *grads,
                                  int num_threads);
RNNTStatus mrnnt_cpu_hat_align(const mrnnt_problem *p, void *workspace, size_t workspace_bytes, int *alignment_out,
                               int64_t out_stride, float *costs, int num_threads);

/* mrnnt_hat_path_forward / _backward and mrnnt_hat_expect_forward / _backward for the host implementation: the
 * arguments, workspace sizes and host checks of mrnnt_cpu_path_* / mrnnt_cpu_expect_*, the formulas, zero-row rule and
 * den' = +inf rule above in fp64 with the library exp / expm1. grads may be acts itself (in place). */
RNNTStatus mrnnt_cpu_hat_path_forward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                      const int *alignments, int num_paths, int64_t path_stride, float *path_costs,
                                      int num_threads);
RNNTStatus mrnnt_cpu_hat_path_backward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                       const int *alignments, int num_paths, int64_t path_stride, const float *weights,
                                       float *grads, int num_threads);
RNNTStatus mrnnt_cpu_hat_expect_forward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                        const float *blank_cost, const float *label_cost, float *expected, float *costs,
                                        int with_grad, int num_threads);
RNNTStatus mrnnt_cpu_hat_expect_backward(const mrnnt_problem *p, void *workspace, size_t workspace_bytes,
                                         const float *blank_cost, const float *label_cost, const float *grad_expected,
                                         const float *grad_costs, float *grads, int num_threads);

/* ---- fused joint network + loss (extension) -------------------------------------
 * The logits are not an input: z(b,t,s,:) = weight * tanh(enc[b,t,:] + pred[b,s,:]) + bias is formed on the
 * matrix cores inside the log-softmax and gradient passes and never stored (bf16 operands, fp32 accumulate).
 * Labels, lengths, blank and costs have the meaning of mrnnt_problem. H must be 128, 256, 384, 512 or 640. */
typedef struct mrnnt_joint_problem {
    int B;
    int V;
    int H;
    int blank;
    const int *T_host;       /* host [B] */
    const int *S_host;       /* host [B] */
    const int *T_dev;        /* device [B] */
    const int *S_dev;        /* device [B] */
    const int *labels;       /* device [B, label_stride] */
    int64_t label_stride;
    const void *enc;         /* device bf16, row (b, t) at enc + b*enc_stride + t*H (elements) */
    int64_t enc_stride;      /* multiple of 8, >= max_b T_b * H */
    const void *pred;        /* device bf16, row (b, s) at pred + b*pred_stride + s*H */
    int64_t pred_stride;     /* multiple of 8, >= (max_b S_b + 1) * H */
    const void *weight;      /* device bf16 [V, H] */
    const float *bias;       /* device fp32 [V] or NULL */
    const int *alignment;    /* device [B, align_stride] or NULL: restriction as in mrnnt_problem */
    int64_t align_stride;
    int align_blank;
    int max_shift;
    int64_t hact_ld;         /* (version 3) Hact row stride in elements, 0 = H; a multiple of 8 > H makes
                                mrnnt_joint_backward write columns H .. hact_ld-1 of every row as [1, 0, ...],
                                so that the dweight GEMM G^T Hact also yields dbias = sum_i G[i] in column H */
    float *dbias;            /* (version 8) device fp32 [V] or NULL: mrnnt_joint_backward ADDS sum_i G[i] (the fp32
                                values before their bf16 rounding) into it -- zero it first; H <= 512 only, and V small
                                enough for its per-wave LDS column sums (mrnnt_joint_backward reports otherwise). Summed
                                in a fixed order: bitwise reproducible (version 9; version 8 used float atomics) */
    void *reduce_scratch;    /* (version 9) device memory for mrnnt_joint_reduce, >= mrnnt_joint_reduce_scratch_bytes,
                                or NULL (a slower one-block-per-utterance form runs); e.g. G once dH = G weight exists */
    size_t reduce_scratch_bytes;
    const unsigned long long *live_count_dev; /* (version 12) device uint64 or NULL: the count mrnnt_joint_live_rows
                                wrote. When set, the n_live argument of mrnnt_joint_backward (and of mrnnt_joint_dpre /
                                mrnnt_joint_reduce / mrnnt_joint_reduce_pre) is a host-known UPPER BOUND on the count
                                (mrnnt_joint_row_bound) and the kernels take the count from this word: no device-to-host
                                read between the forward and the backward, so a training step can be captured in a HIP
                                graph. mrnnt_joint_backward then also writes rows [count, n_live) of G and Hact as zeros,
                                so library GEMMs over all n_live rows (dweight, dH) see zero rows there. */
} mrnnt_joint_problem;

RNNTStatus mrnnt_joint_workspace_size(const mrnnt_joint_problem *p, size_t *bytes);

/* (version 12) A host-known upper bound on the live-row count of mrnnt_joint_live_rows: the lattice rows inside the
 * monotonic band, from the host lengths (no device read). Size G / Hact with it under p->live_count_dev. Unchanged for
 * the factorised-blank calls (mrnnt_joint_hat_*). */
RNNTStatus mrnnt_joint_row_bound(const mrnnt_joint_problem *p, int64_t *rows);

/* Forward: costs_dev[b] = -log P(labels_b | enc_b, pred_b); with_beta as in mrnnt_forward. */
RNNTStatus mrnnt_joint_forward(const mrnnt_joint_problem *p, void *workspace, size_t workspace_bytes,
                               float *costs_dev, int with_beta, hipStream_t stream);

/* mrnnt_align for the fused joint (an addition to version 13: MRNNT_VERSION and both structs are unchanged, so callers
 * that may meet an older build of version 13 probe for the symbols mrnnt_joint_align / mrnnt_joint_posteriors): the
 * best path through the lattice of the logits the joint never stores. Everything mrnnt_joint_forward does up to and
 * including its joint log-softmax pass (p->alignment / p->max_shift restrict the search as they restrict the loss),
 * then the Viterbi launch of mrnnt_align in the recursion's place. The contract is mrnnt_align's: the label arc is
 * taken only when STRICTLY greater than the blank arc; alignment_out_dev[b*out_stride + t] is labels[b, s] or
 * p->blank for t < T_b (the format p->alignment consumes with align_blank == blank) and p->blank for
 * T_b <= t < out_stride; costs_dev[b] (fp32, may be NULL) is the negative log-probability of that path. No finite
 * path: cost +inf and the whole row -1. A NaN or +inf logit inside the utterance's band (e.g. a NaN in its enc rows):
 * cost NaN and the row -1; the other utterances are bit-identical to a call without it.
 * alignment_out_dev != NULL and out_stride >= max_b T_b are checked on the host before any device call
 * (RNNT_STATUS_INVALID_VALUE). p->alignment and alignment_out_dev may be the same buffer (the band is built from the
 * input before the output is written). Workspace: mrnnt_joint_workspace_size bytes; the back-pointers, one bit per
 * cell, use its alpha array, so the call OVERWRITES the state of an earlier mrnnt_joint_forward on that workspace (run
 * the forward again before mrnnt_joint_live_rows / mrnnt_joint_backward / mrnnt_joint_posteriors). The joint launch
 * counts under [5] of mrnnt_profile_read and the Viterbi launch under [2]. Asynchronous on `stream`, no host read. */
RNNTStatus mrnnt_joint_align(const mrnnt_joint_problem *p, void *workspace, size_t workspace_bytes,
                             int *alignment_out_dev, int64_t out_stride, float *costs_dev, hipStream_t stream);

/* mrnnt_posteriors for the fused joint, after mrnnt_joint_forward(with_beta = 1) on the same workspace and inputs:
 * the same values and rules (fp64 formation, unreachable rows exactly 0, a non-finite ll makes that utterance's
 * values NaN and no other's, emit 0 for t >= T_b, label_time -1 for s >= S_b, any output may be NULL, every sum in a
 * fixed order: bitwise reproducible). One difference: a joint caller has no packed row index, so the per-row outputs
 * lie on the joint's own grid,
 *   blank_post_dev / label_post_dev: [B, grid_T, grid_S1], row (b, t, s) at (b*grid_T + t)*grid_S1 + s, the rows
 *       with t >= T_b or s > S_b 0 -- e.g. grid_T / grid_S1 = the frame / label-position slots of enc / pred.
 * grid_T >= max T_b and grid_S1 >= max S_b + 1 (when either per-row output is given), emit_stride >= max T_b and
 * time_stride >= max S_b are checked on the host, with the NULL workspace, before any device call
 * (RNNT_STATUS_INVALID_VALUE). Reads the workspace only; its launch counts under [2] of mrnnt_profile_read.
 * Asynchronous on `stream`, no host read. Works unchanged after mrnnt_joint_hat_forward(with_beta = 1): the posteriors
 * are then those of the factorised-blank distribution. */
RNNTStatus mrnnt_joint_posteriors(const mrnnt_joint_problem *p, const void *workspace, float *blank_post_dev,
                                  float *label_post_dev, int64_t grid_T, int64_t grid_S1, float *emit_dev,
                                  int64_t emit_stride, float *label_time_dev, int64_t time_stride, hipStream_t stream);

/* mrnnt_sample for the fused joint, after mrnnt_joint_forward(with_beta = 1) on the same workspace and inputs: the
 * same walk, random numbers, outputs ([B, num_samples, out_stride] / [B, num_samples]), sentinels and host checks
 * (the joint's lengths are on the host: out_stride >= max T_b is checked here). The same launch on the joint's packed
 * lattice; reads the workspace, labels and the lengths only. Counts under [2] of mrnnt_profile_read. Works unchanged
 * after mrnnt_joint_hat_forward(with_beta = 1): the paths are then drawn from the factorised-blank posterior. */
RNNTStatus mrnnt_joint_sample(const mrnnt_joint_problem *p, const void *workspace, int num_samples, uint64_t seed,
                              int64_t first_sample, int *alignments_dev, int64_t out_stride, float *path_costs_dev,
                              hipStream_t stream);

/* After mrnnt_joint_forward(with_beta=1): list the live lattice rows (those with a non-zero fp32 logit
 * gradient) in the workspace and write their number to *count_dev (device uint64). Works unchanged after
 * mrnnt_joint_hat_forward(with_beta = 1): the threshold is on the row's occupancy cb + ce, which bounds every
 * factorised gradient element, so a row left out is all zero there too (a kept row may still be: time, not results). */
RNNTStatus mrnnt_joint_live_rows(const mrnnt_joint_problem *p, void *workspace, unsigned long long *count_dev,
                                 hipStream_t stream);

/* After mrnnt_joint_live_rows: for live row i (n_live = the count it produced, read back by the caller),
 * G[i, :] = grad_scale[b] * dcost_b/dz (bf16 [n_live, V]), Hact[i, :] = tanh(enc + pred) (bf16 [n_live, H]),
 * bt_idx[i] = b*(enc_stride/H) + t and bs_idx[i] = b*(pred_stride/H) + s (int64; either may be NULL). Then
 * dweight = G^T Hact, dbias = sum_i G[i] (= column H of G^T Hact when hact_ld > H), and with
 * dpre = (G weight) * (1 - Hact^2):
 * denc[bt_idx[i]] += dpre[i], dpred[bs_idx[i]] += dpre[i]. grad_scale may be NULL (= 1). */
RNNTStatus mrnnt_joint_backward(const mrnnt_joint_problem *p, void *workspace, int64_t n_live,
                                const float *grad_scale, void *G, void *Hact, int64_t *bt_idx, int64_t *bs_idx,
                                hipStream_t stream);

/* (version 10) After mrnnt_joint_backward: dpre = (G weight) * (1 - Hact^2), bf16 [n_live, H], on hand-written MFMA
 * tiles (mrnnt_joint_gemm.hip): the dH GEMM with the tanh derivative in its epilogue. weight_t is the weight
 * transposed, bf16 [H, V] row-major; Hact as mrnnt_joint_backward wrote it (row stride p->hact_ld, 0 = H). Needs
 * H = 256 or 512 and V a multiple of 8 (RNNT_STATUS_INVALID_VALUE otherwise: use a library GEMM for dH and
 * mrnnt_joint_reduce with Hact). Sum dpre with mrnnt_joint_reduce_pre. Works unchanged after
 * mrnnt_joint_hat_backward. */
RNNTStatus mrnnt_joint_dpre(const mrnnt_joint_problem *p, int64_t n_live, const void *G, const void *weight_t,
                            const void *Hact, void *dpre, hipStream_t stream);

/* After mrnnt_joint_backward, with dH = G weight (bf16 [n_live, H], e.g. a library GEMM): accumulate
 * dpre = dH * (1 - Hact^2) into d_enc (fp32, enc's [B, enc_stride/H, H] shape; rows (b, t < T_b) are
 * overwritten) and d_pred (fp32, pred's shape; added to: zero it first). Zero d_enc's padding rows yourself.
 * Hact is required (RNNT_STATUS_INVALID_VALUE when NULL with n_live > 0). Every sum has a fixed order (bitwise reproducible). p->reduce_scratch (version 9) lets it run on blocks of frames
 * whose d_pred sums are then added in block order; see mrnnt_joint_reduce_scratch_bytes. Works unchanged after
 * mrnnt_joint_hat_backward (as does mrnnt_joint_reduce_pre). */
RNNTStatus mrnnt_joint_reduce(const mrnnt_joint_problem *p, void *workspace, int64_t n_live, const void *dH,
                              const void *Hact, float *d_enc, float *d_pred, hipStream_t stream);

/* (version 11) mrnnt_joint_reduce for a dH that already holds dpre = dH * (1 - Hact^2) (mrnnt_joint_dpre's output,
 * bf16 [n_live, H]): the same sums of dpre into d_enc / d_pred, in the same fixed order. (Version 10 signalled this
 * with Hact = NULL on mrnnt_joint_reduce, which made a forgotten Hact a silent wrong gradient.) */
RNNTStatus mrnnt_joint_reduce_pre(const mrnnt_joint_problem *p, void *workspace, int64_t n_live, const void *dpre,
                                  float *d_enc, float *d_pred, hipStream_t stream);

/* (version 9) Bytes of p->reduce_scratch for the blocked form of mrnnt_joint_reduce. */
RNNTStatus mrnnt_joint_reduce_scratch_bytes(const mrnnt_joint_problem *p, size_t *bytes);

/* mrnnt_path_forward / mrnnt_path_backward for the fused joint (an addition to version 13: MRNNT_VERSION and both
 * structs are unchanged, so callers that may meet an older build of version 13 probe for the symbol
 * mrnnt_joint_path_forward): differentiable scores of num_paths GIVEN alignments per utterance under the logits the
 * joint never stores, and the gradients of sum_{b,k} w[b, k] * path_costs[b, k] for enc, pred, weight and bias through
 * the joint's own backward chain over the rows the paths stand on -- at most num_paths * T_b per utterance -- with no
 * dense logit gradient at all. The contract of mrnnt_path_*, stated once more for the joint:
 *   alignments_dev[(b*num_paths + k)*path_stride + t], t < T_b: p->blank or the label frame t emits (the format
 *       mrnnt_joint_align / mrnnt_joint_sample write); entries at t >= T_b are not read.
 *   Row (b, k) is walked from s = 0: p->blank takes the blank arc of row (t, s); labels[b, s] with s < S_b takes the
 *       label arc, then s += 1; anything else (a wrong or negative value, the -1 sentinel rows, a label at s = S_b), or
 *       s != S_b after frame T_b - 1, makes the row INVALID: it costs +inf and contributes nothing whatever its weight.
 *   path_costs_dev[b*num_paths + k] (may be NULL) = fp32(-sum_t lp(arc_t)), lp the pairs mrnnt_joint_forward leaves in
 *       the workspace (the same kernel on the same operands; an out-of-range device label: NaN), summed in fp64 in the
 *       fixed order of mrnnt_path_forward. Only the rows between the lowest and the highest valid path of each frame
 *       (the hull) are computed, plus row (0, 0) of an utterance without a valid path. No recursion runs.
 *   With Wb(r) / We(r) the fp64 sums, in ascending k, of the weights of the VALID paths that leave row r by its blank /
 *       label arc, the logit gradient of row r is mrnnt_path_backward's,
 *           g[r, v] = (Wb + We) softmax(z_r)[v] - [v == blank] Wb - [v == label(s)] We.
 *       A row with Wb == 0 && We == 0 is not in the backward's row list; Wb == -We != 0 is a live row whose softmax
 *       term cancels and whose two corrections stay.
 *   Costs and all four gradients are bitwise reproducible.
 * Calls, on one workspace of mrnnt_joint_path_workspace_size(p, num_paths) bytes:
 *   mrnnt_joint_path_forward: walk + hull, the list of the hull rows (its count stays on the device), the joint
 *       log-softmax pass over that list, the score launch.
 *   mrnnt_joint_path_rows (after it, same alignments): weights_dev[b*num_paths + k] (fp32, signed; NULL = 1) is the
 *       upstream gradient of path_costs; the coefficient launch, then the list of the path-live rows (inside the hull,
 *       Wb != 0 || We != 0) with its count in *count_dev (device uint64). mrnnt_joint_path_row_bound is a host-known
 *       upper bound on that count: sum_b min(num_paths * T_b, in-band rows of b).
 *   mrnnt_joint_path_backward: mrnnt_joint_backward over that list with the path coefficients in place of the loss's
 *       (no grad_scale: the weights are in Wb / We). G, Hact, bt_idx, bs_idx, p->hact_ld, p->dbias and
 *       p->live_count_dev (n_rows then a host bound, rows [count, n_rows) zeroed) as there.
 *   Then mrnnt_joint_dpre / mrnnt_joint_reduce / mrnnt_joint_reduce_pre exactly as after mrnnt_joint_backward: the
 *       workspace is laid out as mrnnt_joint_workspace_size's of the same problem FOLLOWED by the hull arrays and a few
 *       words per path, so those entry points work on it unchanged (the reduce takes its column offsets from the last
 *       list built, the path-live one).
 * Checked on the host before any device call, workspace included (RNNT_STATUS_INVALID_VALUE): p->alignment == NULL
 * (the band arrays hold the hull); num_paths >= 1; alignments_dev != NULL; path_stride >= max T_b; everything
 * mrnnt_joint_workspace_size checks. Asynchronous on `stream`, no host read. The walk, score and coefficient launches
 * count under [2] of mrnnt_profile_read, the joint pass under [5], the gradient pass under [6]. */
RNNTStatus mrnnt_joint_path_workspace_size(const mrnnt_joint_problem *p, int num_paths, size_t *bytes);
RNNTStatus mrnnt_joint_path_row_bound(const mrnnt_joint_problem *p, int num_paths, int64_t *rows);
RNNTStatus mrnnt_joint_path_forward(const mrnnt_joint_problem *p, void *workspace, size_t workspace_bytes,
                                    const int *alignments_dev, int num_paths, int64_t path_stride,
                                    float *path_costs_dev, hipStream_t stream);
RNNTStatus mrnnt_joint_path_rows(const mrnnt_joint_problem *p, void *workspace, size_t workspace_bytes,
                                 const int *alignments_dev, int num_paths, int64_t path_stride,
                                 const float *weights_dev, unsigned long long *count_dev, hipStream_t stream);
RNNTStatus mrnnt_joint_path_backward(const mrnnt_joint_problem *p, void *workspace, int64_t n_rows, void *G, void *Hact,
                                     int64_t *bt_idx, int64_t *bs_idx, hipStream_t stream);

/* mrnnt_expect_forward / mrnnt_expect_backward for the fused joint (an addition to version 13: MRNNT_VERSION and both
 * structs are unchanged, so callers that may meet an older build of version 13 probe for the symbol
 * mrnnt_joint_expect_forward): the exact expectation of an arc-additive cost under the logits the joint never stores,
 * and the gradients of sum_b g_e[b] expected[b] + g_c[b] costs[b] for enc, pred, weight and bias through the joint's
 * own backward chain -- ONE set of row coefficients over ONE row list, whatever the two upstream gradients are. The
 * contract is that of mrnnt_expect_* above (A, Bk, R, cb, ce as defined there), stated for the joint:
 *   blank_cost_dev / label_cost_dev: wb / we, fp32 [B, grid_T, grid_S1], row (b, t, s) at (b*grid_T + t)*grid_S1 + s
 *       -- the grid mrnnt_joint_posteriors writes blank_post / label_post on; grid_T >= max T_b, grid_S1 >= max S_b + 1.
 *       Either may be NULL (all zeros; with both NULL the grid is not looked at). we at s = S_b, and anything at
 *       t >= T_b or s > S_b, never enters a result. The cost arrays are not differentiated.
 *   Wb = g_c blank_post - g_e cb,   We = g_c label_post - g_e ce     (fp64, the function of mrnnt_expect_backward)
 *   g[r, v] = (Wb + We) softmax(z_r)[v] - [v == blank] Wb - [v == label(s)] We     (mrnnt_joint_path_backward's formula)
 *   A row whose two fp32 coefficients are both zero is not in the backward's row list. An utterance whose ll is not
 *   finite has expected[b] NaN and every row of its monotonic band listed with NaN coefficients (as mrnnt_joint_backward
 *   treats it); the other utterances' expected and costs are bit-identical to a call without it. With p->alignment the
 *   expectation is under the restricted distribution. Every sum has a fixed order, no atomics: expected, costs and all
 *   four gradients are bitwise reproducible.
 * Calls, on one workspace of mrnnt_joint_expect_workspace_size(p) bytes:
 *   mrnnt_joint_expect_forward: mrnnt_joint_forward(with_beta = with_grad) (costs_dev: the loss, bit for bit), then
 *       the expectation recursion of mrnnt_expect_forward on the joint's packed lattice; expected_dev[b] = fp32(R)
 *       (either output may be NULL).
 *   mrnnt_joint_expect_rows (after it with with_grad = 1; the same cost arrays and grid): grad_expected_dev /
 *       grad_costs_dev are fp32 [B], either may be NULL = 0 for that term; one coefficient launch writes Wb / We of
 *       every row of the monotonic band (exact 0.0 for a dead row), then the list of the expect-live rows (Wb != 0 ||
 *       We != 0, column order, s ascending) with its count in *count_dev (device uint64). mrnnt_joint_row_bound is the
 *       host-known bound on that count.
 *   mrnnt_joint_expect_backward: mrnnt_joint_path_backward's gradient pass over that list, reading Wb / We from the two
 *       arrays. G, Hact, bt_idx, bs_idx, p->hact_ld, p->dbias and p->live_count_dev as there.
 *   Then mrnnt_joint_dpre / mrnnt_joint_reduce / mrnnt_joint_reduce_pre exactly as after mrnnt_joint_backward: the
 *       workspace is laid out as mrnnt_joint_workspace_size's of the same problem FOLLOWED by A, Bk (fp64 [N]), R (fp64
 *       [B]) and Wb, We (fp64 [N]), so those entry points work on it unchanged.
 * Checked on the host before any device call (RNNT_STATUS_INVALID_VALUE): everything mrnnt_joint_forward checks; a
 * grid smaller than [max T, max S + 1] when either cost array is given; a NULL or too small workspace; a NULL
 * count_dev. Asynchronous on `stream`, no host read. The recursion and coefficient launches count under [2] of
 * mrnnt_profile_read, the joint pass under [5], the gradient pass under [6]. */
RNNTStatus mrnnt_joint_expect_workspace_size(const mrnnt_joint_problem *p, size_t *bytes);
RNNTStatus mrnnt_joint_expect_forward(const mrnnt_joint_problem *p, void *workspace, size_t workspace_bytes,
                                      const float *blank_cost_dev, const float *label_cost_dev, int64_t grid_T,
                                      int64_t grid_S1, float *expected_dev, float *costs_dev, int with_grad,
                                      hipStream_t stream);
RNNTStatus mrnnt_joint_expect_rows(const mrnnt_joint_problem *p, void *workspace, size_t workspace_bytes,
                                   const float *blank_cost_dev, const float *label_cost_dev, int64_t grid_T,
                                   int64_t grid_S1, const float *grad_expected_dev, const float *grad_costs_dev,
                                   unsigned long long *count_dev, hipStream_t stream);
RNNTStatus mrnnt_joint_expect_backward(const mrnnt_joint_problem *p, void *workspace, int64_t n_rows, void *G,
                                       void *Hact, int64_t *bt_idx, int64_t *bs_idx, hipStream_t stream);

/* mrnnt_hat_forward / mrnnt_hat_backward / mrnnt_hat_align for the fused joint (an addition to version 13:
 * MRNNT_VERSION and both structs are unchanged, so callers that may meet an older build of version 13 probe for the
 * symbol mrnnt_joint_hat_forward): the factorised-blank (HAT) loss of the logits the joint never stores. Blank is a
 * Bernoulli on its own logit z_b and the labels a softmax over the other V - 1 logits,
 *   lpb = log sigmoid(z_b),   lpe = log sigmoid(-z_b) + z_l - LSE_{v != b} z_v,
 * with the rules of mrnnt_hat_forward: the blank logit is masked out of the row's max and sum (never subtracted
 * afterwards); z_b = +inf or a NaN / +inf logit anywhere in the row makes both NaN; a label equal to blank is no arc; a
 * row whose non-blank logits are all -inf has no label arc and an untouched blank arc. The logit gradient is
 *   g[b] = ce sigmoid(z_b) - cb sigmoid(-z_b),   g[v != b] = ce (exp(z_v - LSE_{u != b} z_u) - [v == label(s)])
 * times grad_scale, cb / ce the blank / label arc posteriors of the row.
 *   mrnnt_joint_hat_forward: mrnnt_joint_forward with the factorised-blank joint pass; same workspace
 *       (mrnnt_joint_workspace_size), arguments, host checks and alignment restriction.
 *   mrnnt_joint_hat_align: mrnnt_joint_align under the factorised probabilities; same contract and host checks.
 *   mrnnt_joint_hat_backward: mrnnt_joint_backward with the factorised-blank row coefficients, after
 *       mrnnt_joint_hat_forward(with_beta = 1) and mrnnt_joint_live_rows on the same workspace. G, Hact, bt_idx, bs_idx,
 *       grad_scale, p->hact_ld, p->dbias and p->live_count_dev (n_live then a host bound, rows [count, n_live) zeroed)
 *       as there. Every factorised gradient element is at most cb + ce in magnitude, the occupancy the live-row list
 *       thresholds, so a row it leaves out is all zero in fp32. An utterance without a path (ll = -inf, cost +inf)
 *       gets exact zeros in its rows of G -- not the NaN of mrnnt_joint_backward / mrnnt_hat_backward -- so that it
 *       does not turn dweight and dbias, which sum over the batch, into NaN; a NaN cost keeps NaN gradients.
 * mrnnt_joint_posteriors, mrnnt_joint_sample, mrnnt_joint_live_rows, mrnnt_joint_reduce, mrnnt_joint_reduce_pre,
 * mrnnt_joint_dpre and mrnnt_joint_row_bound work unchanged after mrnnt_joint_hat_forward(with_beta = 1): they read the
 * recursion's state and the row lists, never the logits or the meaning of the denominator. Costs and all four
 * gradients are bitwise reproducible. The launches count under mrnnt_profile_read as those of mrnnt_joint_*. */
RNNTStatus mrnnt_joint_hat_forward(const mrnnt_joint_problem *p, void *workspace, size_t workspace_bytes,
                                   float *costs_dev, int with_beta, hipStream_t stream);
RNNTStatus mrnnt_joint_hat_backward(const mrnnt_joint_problem *p, void *workspace, int64_t n_live,
                                    const float *grad_scale, void *G, void *Hact, int64_t *bt_idx, int64_t *bs_idx,
                                    hipStream_t stream);
RNNTStatus mrnnt_joint_hat_align(const mrnnt_joint_problem *p, void *workspace, size_t workspace_bytes,
                                 int *alignment_out_dev, int64_t out_stride, float *costs_dev, hipStream_t stream);

/* Nontemporal zero fill of `bytes` (a multiple of 16) at `dst` (16-byte aligned device memory), in the gradient
 * pass's store pattern. The Python surface times it once over a newly allocated large grads buffer to pick a
 * fast-writing physical placement; also usable as a plain fill. Asynchronous on `stream`. */
RNNTStatus mrnnt_fill_zero(void *dst, size_t bytes, hipStream_t stream);

int mrnnt_version(void);

/* Kernel-time accounting over HIP events recorded around each launch on its stream.
 * enable=1 starts recording (clearing previous records). mrnnt_profile_read synchronises the
 * recorded events and returns per-kernel totals in ms and launch counts for
 *   [0] band, [1] log-softmax row reduce, [2] alpha/beta DP, [3] logit gradient, [4] setup,
 *   [5] joint forward, [6] joint backward, [7] joint reduce, [8] chase launch (log-softmax + alpha/beta),
 *   [9] joint dpre GEMM (version 10). mrnnt_align's Viterbi launch, mrnnt_posteriors and mrnnt_sample count under [2],
 *   and so do the walk, score and coefficient launches of mrnnt_path_forward / mrnnt_path_backward (their log-softmax
 *   under [1], their gradient under [3]) and the recursion launch of mrnnt_expect_forward (the gradient of
 *   mrnnt_expect_backward under [3]) and the recursion and coefficient launches of mrnnt_joint_expect_*. */
void mrnnt_profile_enable(int enable);
int mrnnt_profile_read(double *total_ms, int64_t *launches, int n);

#ifdef __cplusplus
}
#endif

#endif /* MONOTONIC_RNNT_MRNNT_H */
