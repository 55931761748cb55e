/* m2d.h — C-ABI of libm2d_hip.so: the MI355X (gfx950) kernels behind the WGAN-GP hot
 * path of clementabary/music2dance.
 *
 * The reference has no FFI of its own: it is pure Python on stock PyTorch ops. Each entry
 * point below therefore replaces the stock op that the cited reference line calls, and is
 * what a maintainer would bind (ctypes stub in INTEGRATION.md) to move that op onto the
 * hand-written CDNA4 kernels.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 (int32 for `lengths`) owned by the caller;
 *     the one exception is the cross-entropy family, whose `labels` and `pred` are int64
 *     (torch's class-index dtype);
 *     tensors are dense row-major in the reference's own layouts: activations (B, C, L),
 *     conv weights (Cout, Cin, k), linear weights (out, in), sequences (B, T, H);
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue on it: no allocation,
 *     no host synchronisation, safe under hipGraph stream capture;
 *   - `ws` / `ws_bytes`: scratch sized by the matching *_workspace_bytes() query;
 *   - return 0 on success, a negative M2D_ERR_* code otherwise (m2d_last_error() gives the
 *     thread-local message); nothing throws across the boundary;
 *   - `act`: 0 none, 1 ReLU, 2 LeakyReLU(slope). A `*_mask` argument multiplies an operand
 *     or the result by (mask > 0 ? 1 : mask_slope) — the derivative of the fused
 *     activation — which closes the op set under differentiation for the gradient
 *     penalty's double backward (losses.py:40-44).
 *   - operand alignment ("Operand alignment"): every float operand needs its natural 4-byte alignment
 *     and no more (int64 labels 8 bytes, bytes none), unless the entry's comment says otherwise - today the STFT basis
 *     image, the JPEG workspace, m2d_maxpool2_fwd_from's sample starts and m2d_sync_scan's `r`; an `out` / `sum_out`
 *     view one float into a buffer is as good as a fresh allocation. Inside the library:
 *       . plain global loads and stores (to or from registers) may be issued 16 bytes wide at 4-byte alignment - the
 *         sub-pixel backward-data epilogue does so in every training step (its addresses are 4 q - pad);
 *       . LDS-DMA wider than 4 bytes, and anything that derives an LDS address or bank layout from a global
 *         address, is selected only when the source pointer and every row start are 16-byte aligned; the routing
 *         tests the pointers and takes a narrower kernel otherwise (a direct call of a kernel-specific entry point
 *         such as m2d_conv1d_fwd_k4 fails with M2D_ERR_ARG instead: it has no other kernel to take).
 */
#ifndef M2D_H
#define M2D_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define M2D_OK 0
#define M2D_ERR_ARG -1
#define M2D_ERR_HIP -2
#define M2D_ERR_WORKSPACE -3
#define M2D_ERR_RANGE -4

/* ---- runtime ------------------------------------------------------------------------ */
const char* m2d_last_error(void);
int m2d_version(void);
/* HIP-event profiler used by bench.py: per kernel family {ms, launches, flops, bytes}.
 * Families: 0 gemm engine, 1 batch-norm, 2 gru, 3 pointwise, 4 reductions. */
int m2d_prof_begin(void);
int m2d_prof_end(double* out, int n_out /* >= 20 */);
/* per-launch CSV "family,tag,d0,d1,d2,ms,flops,bytes" of the current session; call before m2d_prof_end */
int m2d_prof_dump(char* buf, int cap);
/* GEMM-engine launch plans (tile height, split-K factor) come from a cost model: nothing is timed, a shape's plan is a
 * pure function of the shape, the workspace and the stream's ticket scratch.
 * Round 5: which cost model ranks the plans. 4 (default): the
 * round-4 model; 5: chunk-step floor by tile height and up to 256 splits - faster launch by launch, slower where the
 * streams of a loop body overlap. Process-wide; M2D_PLAN_MODEL=4|5 sets the initial value. */
int m2d_plan_model_set(int model);
int m2d_plan_model_get(void);

/* ---- conv1d: nn.Conv1d forward and both halves of its backward -------------------------
 * reference: phase3/archis/default.py:64-70 (DefaultAudioEncoder), :90-97,216 (U-Net),
 * :117-128 (WaveGAN), :201-204 (TemporalBlock), :298-303 (AudioDiscriminator),
 * :326-333 (StickDiscriminator); phase2/archis/default.py:31-38,154-157. */
/* `stats` (optional, 2*Cout doubles, zeroed by the call): stats[2c] += sum, stats[2c+1] += sum of squares of
 * the stored y[:, c, :] - the batch statistics a following BatchNorm needs (m2d_bn_fwd_sums), taken in the
 * conv's epilogue instead of a second pass over y. */
int m2d_conv1d_fwd(const float* x, const float* w, const float* w_packed, const float* bias, float* y, int B,
                   int Cin, int L, int Cout, int ks, int stride, int pad, int act, float slope,
                   const float* residual, const float* out_mask, float out_mask_slope, double* stats, void* ws,
                   size_t ws_bytes, void* stream);
/* `out_mask` (optional, shape of dx): the result is multiplied by (mask>0 ? 1 : out_mask_slope) in the
 * epilogue - the activation derivative of the layer that produced x, so that a chain of fused
 * conv + ReLU layers hands each other gradients that are already masked (no masked operand loads). */
int m2d_conv1d_bwd_data(const float* dy, const float* w, const float* w_packed, float* dx, int B, int Cin, int L,
                        int Cout, int ks, int stride, int pad, const float* dy_mask, float dy_mask_slope,
                        const float* out_mask, float out_mask_slope, void* ws, size_t ws_bytes, void* stream);
/* `dbias` (optional, Cout floats): sum over (batch, length) of dy (masked like dy) - the bias gradient -
 * from the same launch (an all-ones column appended to the x operand), instead of a second pass over dy. */
int m2d_conv1d_bwd_weight(const float* x, const float* dy, float* dw, float* dbias, int B, int Cin, int L,
                          int Cout, int ks, int stride, int pad, const float* dy_mask, float dy_mask_slope,
                          void* ws, size_t ws_bytes, void* stream);
/* ---- the critic iteration as ONE hand-scheduled pass (round 3; music2dance_amd/critic_step.py) ---------------
 * The reference runs three critic forwards and three autograd passes per iteration (phase3/train.py:204-216,
 * losses.py:28-44). Scheduled by hand, the pose branch sees ONE batch of 3B rows [interpolated | real | fake], the
 * first backward of the penalty and the loss backward travel together, and every weight gradient of a layer comes
 * from one launch. The entry points below are what that schedule needs on top of the three conv ops:
 *  - m2d_conv1d_fwd_sum: two outputs, y = out_mask * act(conv + bias) and sum_out = y + residual (a TemporalBlock's
 *    second conv, phase3/archis/default.py:207-210: relu(conv) is the backward mask, x + relu(conv) the next input).
 *    m2d_conv1d_fwd itself applies out_mask BEFORE its residual (out = act'(y) * conv(g) + skip: the forward-mode
 *    tangent of a skip block).
 *  - m2d_conv1d_bwd_data_res: dx = out_mask * (conv^T(dy) + residual) - the skip connection's gradient is added in
 *    the epilogue instead of by an accumulation pass.
 *  - m2d_conv1d_bwd_weight_from: the bias gradient sums over samples [bias_from_sample, B) only, so rows that pair
 *    second-order operands (no bias term) can share the launch with ordinary (x, dy) rows.
 *  - m2d_gemm_ld: m2d_gemm on sub-matrices of wider buffers (row pitches lda / ldb / ldc in elements, 0 = dense;
 *    a_mask shares lda, out_mask shares ldc): the (B, 200) concatenated code of phase3/archis/default.py:266-269
 *    is written / read in place.
 *  - m2d_pose_pack3: (3B, C, T) = [alpha*real + (1-alpha)*fake | real^T | fake^T] from real (B, T, C) and the
 *    generator's rows (B*T, C): phase3/train.py:196-199 + losses.py:13-25 in one LDS-staged transpose.
 *  - m2d_wgan_critic_loss: out[0..2] = (E[D(fake)] - E[D(real)] + gamma*gp, gp, E[D(fake)] - E[D(real)]) from the
 *    (3B,) scores and the penalty term(s) (phase3/train.py:210-212). */
int m2d_conv1d_fwd_sum(const float* x, const float* w, const float* w_packed, const float* bias, float* y,
                       float* sum_out, int B, int Cin, int L, int Cout, int ks, int stride, int pad, int act,
                       float slope, const float* residual, const float* out_mask, float out_mask_slope, void* ws,
                       size_t ws_bytes, void* stream);
/* Tap-vectorised stride-4 forward (round 3): for the audio critic's k25 / s4 layers (phase3/archis/default.py:298-303)
 * the four taps 4g..4g+3 of one output position are 16 aligned bytes of x and consecutive positions are 16 bytes
 * apart, so the conv's B operand is staged with `buffer_load_dwordx4 ... lds` (a contiguous kilobyte per wave) and
 * read back as ds_read_b128 fragments; weights come from the packed image Wk4[tap group][Cout][4]
 * (m2d_conv1d_pack_weights_k4, m2d_conv1d_k4_packed_elems floats; phantom taps are zeros; the ORDER of the tap groups
 * is private to the pack / forward pair - k25 / pad 11 layers walk the full groups first and the partial first / last
 * groups of four channels together, so that the zero slots are never multiplied). Same results as
 * m2d_conv1d_fwd up to summation order; m2d_conv1d_k4_applicable says whether a layer qualifies (stride 4,
 * L % 4 == 0, Cin % 4 == 0, Cin >= 16, Cout >= 64) BY ITS SHAPE; the pointers are the caller's to test: x and w_k4
 * must be 16-byte aligned (the 16-byte LDS-DMA reads them; with L % 4 == 0 every row of x then is) - m2d_conv1d_fwd_k4
 * fails with M2D_ERR_ARG before it launches otherwise, and m2d_conv1d_fwd serves such an x.
 * sum_out: optional second output as in m2d_conv1d_fwd_sum. */
int m2d_conv1d_k4_applicable(int Cin, int L, int Cout, int ks, int stride, int pad);
size_t m2d_conv1d_k4_packed_elems(int Cout, int Cin, int ks, int pad);
int m2d_conv1d_pack_weights_k4(const float* w, float* out, int Cout, int Cin, int ks, int pad, void* stream);
int m2d_conv1d_fwd_k4(const float* x, const float* w_k4, const float* bias, float* y, float* sum_out, int B, int Cin,
                      int L, int Cout, int ks, int stride, int pad, int act, float slope, const float* residual,
                      const float* out_mask, float out_mask_slope, double* stats, void* ws, size_t ws_bytes,
                      void* stream);
int m2d_conv1d_bwd_data_res(const float* dy, const float* w, const float* w_packed, float* dx, int B, int Cin, int L,
                            int Cout, int ks, int stride, int pad, const float* dy_mask, float dy_mask_slope,
                            const float* residual, const float* out_mask, float out_mask_slope, void* ws,
                            size_t ws_bytes, void* stream);
int m2d_conv1d_bwd_weight_from(const float* x, const float* dy, float* dw, float* dbias, int B, int Cin, int L,
                               int Cout, int ks, int stride, int pad, const float* dy_mask, float dy_mask_slope,
                               int bias_from_sample, void* ws, size_t ws_bytes, void* stream);
/* Round 5. Advance BatchNorm running buffers once more with batch statistics (raw fp64 sums, as m2d_bn_stats / a conv's
 * epilogue deliver them) they were already advanced with: what a second training-mode forward of the same batch through
 * the same weights leaves behind, without the forward (phase3/train.py:195 + :222: the loop body that holds a generator
 * iteration runs the generator twice on one batch; its audio path is the same both times). tmp: 2 C floats. */
int m2d_bn_update_running(const double* sums, double count, float* running_mean, float* running_var, float* tmp, int C,
                          float eps, float momentum, void* stream);
/* Round 5. m2d_conv1d_bwd_data over a batch whose two halves pass through the SAME activation masks: `out_mask` holds
 * mask_batch samples (B / 2 <= mask_batch <= B); sample n >= mask_batch of dx is masked by mask sample n - mask_batch.
 * The audio branch of the phase-3 critic (phase3/archis/default.py:312-319) is evaluated on the same audio for the
 * interpolated, real and fake poses, so the penalty's first backward (losses.py:40-44) and the loss backward
 * (phase3/train.py:215) run through identical ReLU masks: ONE launch per layer over 2B gradient rows. */
int m2d_conv1d_bwd_data_shared_mask(const float* dy, const float* w, const float* w_packed, float* dx, int B, int Cin,
                                    int L, int Cout, int ks, int stride, int pad, const float* out_mask,
                                    float out_mask_slope, int mask_batch, void* ws, size_t ws_bytes, void* stream);
int m2d_gemm_ld(int mode, const float* a, int lda, const float* b, int ldb, const float* bias, float* c, int ldc,
                int M, int N, int K, int act, float slope, const float* a_mask, float a_mask_slope,
                const float* out_mask, float out_mask_slope, void* ws, size_t ws_bytes, void* stream);
/* nn.Tanh of the `activ: tanh` heads (phase3/archis/default.py:75-76,102-103,134-135,309-310,339-340) and the two
 * derivatives the penalty's double backward needs: gx = gy (1 - y^2); d gx / d y = -2 y g gy (d gx / d gy is
 * m2d_tanh_bwd itself, applied to g). */
int m2d_tanh_fwd(const float* x, float* y, size_t n, void* stream);
int m2d_tanh_bwd(const float* gy, const float* y, float* gx, size_t n, void* stream);
int m2d_tanh_bwd_bwd(const float* g, const float* gy, const float* y, float* g_y, size_t n, void* stream);
int m2d_pose_pack3(const float* real, const float* fake, const float* alpha, float* out, int B, int T, int C,
                   void* stream);
int m2d_wgan_critic_loss(const float* scores, int B, const float* pen0, const float* pen1, float gamma, float* out,
                         void* stream);
/* Audio slicing fused into the first encoder conv (reference: utils.slice_audio_batch, utils.py:329-353,
 * then Conv1d(1, Cout, ...) on the (B*T, 1, window) slices, phase3/archis/default.py:27-28,64,90,117):
 * the windows are read in place from the padded track (B, S) - window t of track b is
 * track[b, t*hop : t*hop + window] - and never written. y / dy: (B*T, Cout, Lout). Workspace: as
 * m2d_conv1d_workspace_bytes(0 / 2, B*T, 1, window, ...). */
int m2d_conv1d_fwd_windows(const float* track, int B, int S, int T, int hop, int window, const float* w,
                           const float* bias, float* y, int Cout, int ks, int stride, int pad, int act, float slope,
                           double* stats, void* ws, size_t ws_bytes, void* stream);
int m2d_conv1d_bwd_weight_windows(const float* track, int B, int S, int T, int hop, int window, const float* dy,
                                  float* dw, float* dbias, int Cout, int ks, int stride, int pad,
                                  const float* dy_mask, float dy_mask_slope, void* ws, size_t ws_bytes, void* stream);
/* The GEMMs behind forward / backward-data contract over (tap, channel) and read the weights
 * through K-major packed images (the GEMM's row index contiguous, so that weight tiles are staged with
 * lane-consecutive loads straight into the LDS): w_fwd (Cin, ks, Cout) and w_bwd (Cout, ks, Cin) of w (Cout, Cin, ks).
 * `w_packed` above is the matching image, or NULL: the call then packs into its workspace.
 * Callers that reuse weights across calls pack once per weight update (either output may be NULL). */
int m2d_conv1d_pack_weights(const float* w, float* w_fwd, float* w_bwd, int Cout, int Cin, int ks, void* stream);
/* which: 0 forward, 1 backward-data, 2 backward-weight (includes the room to pack the weights) */
size_t m2d_conv1d_workspace_bytes(int which, int B, int Cin, int L, int Cout, int ks, int stride, int pad);

/* ---- dense GEMMs behind nn.Linear and the GRU input projection --------------------------
 * reference: phase3/archis/default.py:153,161,176-177,256-257,352;
 * phase1/archis/residual.py:11,19,35,41,54-55.
 * mode 0: C[M,N] = A[M,K] B[N,K]^T + bias[N]; mode 1: C = A[M,K] B[K,N]; mode 2: C = A[K,M]^T B[K,N] */
int m2d_gemm(int mode, const float* a, const float* b, const float* bias, float* c, int M, int N, int K,
             int act, float slope, const float* a_mask, float a_mask_slope, const float* out_mask,
             float out_mask_slope, void* ws, size_t ws_bytes, void* stream);
size_t m2d_gemm_workspace_bytes(int mode, int M, int N, int K);
/* Optional, once per stream: `zeroed` = a device buffer of `bytes` the caller zeroed and keeps alive. Split-K launches
 * (convs and GEMMs above) on that stream then finish in ONE launch: partial tiles meet through per-tile arrival counters
 * taken from this buffer and left zero (m2d_splitk_fixup in csrc/gemm_engine.hip) instead of a second reduction launch.
 * 4 bytes per output tile (64 KB covers every shape of the reference). zeroed == NULL unregisters. Launches of one
 * stream run in order, so streams must not share a buffer. Without it: the two-launch form, no state between calls. */
int m2d_stream_scratch_set(void* stream, void* zeroed, size_t bytes);
/* A HIP stream of the library's own (hipStreamCreateWithFlags, non-blocking), never destroyed: the host side wraps it
 * (torch.cuda.ExternalStream) for its host -> device staging copies - a stream that no framework stream pool can hand out
 * a second time (no reference counterpart: launch plumbing). */
int m2d_stream_create(void** stream);

/* ---- BatchNorm1d (train/eval forward, train backward) + per-channel sums -----------------
 * reference: phase3/archis/default.py:65,68,91,94,118-127,154,179-180,217. */
size_t m2d_bn_workspace_bytes(int C);
/* `scratch` (optional, every reducing call below): m2d_bn_scratch_bytes(C) bytes the caller zeroed ONCE and owns per
 * stream. A call that gets it accumulates there, lets the block that arrives last finish the op (mean / invstd /
 * running buffers; dgamma / dbeta; the float sums) and leaves the scratch zeroed again: one launch instead of memset +
 * reduce + finalize. Two streams must not share a scratch. NULL: the three-launch form, no state between calls. */
size_t m2d_bn_scratch_bytes(int C);
int m2d_bn_fwd(const float* x, const float* gamma, const float* beta, float* running_mean,
               float* running_var, float* y, float* save_mean, float* save_invstd, int B, int C, int L,
               float eps, float momentum, int training, int act, float slope, const float* residual, void* ws,
               size_t ws_bytes, void* scratch, void* stream);
int m2d_bn_bwd(const float* dy, const float* x, const float* gamma, const float* beta, const float* save_mean,
               const float* save_invstd, float* dx, float* dgamma, float* dbeta, int B, int C, int L, int act,
               float slope, void* ws, size_t ws_bytes, void* scratch, void* stream);
/* The same in two halves, statistics as raw fp64 sums (sums[2c] = sum x, sums[2c+1] = sum x^2 over `count`
 * elements per channel; backward: sum dz, sum dz*xhat). Lets a producing conv supply the forward sums
 * (m2d_conv1d_fwd `stats`) and lets data-parallel ranks all-reduce them between the halves
 * (synchronised BatchNorm: global-batch statistics; `count` is then the global element count,
 * `sums_global` the all-reduced buffer, `sums_local` this rank's own for dgamma / dbeta). */
int m2d_bn_stats(const float* x, double* sums, int B, int C, int L, void* scratch, void* stream);
int m2d_bn_fwd_sums(const float* x, const double* sums, double count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float* y, float* save_mean, float* save_invstd, int B,
                    int C, int L, float eps, float momentum, int act, float slope, const float* residual,
                    void* stream);
/* m2d_bn_fwd / m2d_bn_fwd_sums with y_batch_stride elements between consecutive samples of y (0 or C * L: dense). A
 * larger stride writes the result into a channel block of a wider (B, C', L) buffer: the U-Net's skip concatenations
 * (torch.cat((upsample(d), skip), 1), phase3/archis/default.py:240-245) are then produced in place - the skip's
 * BatchNorm and m2d_upsample2_fwd_to write the two halves, no cat pass over both. */
int m2d_bn_fwd_to(const float* x, const float* gamma, const float* beta, float* running_mean,
                  float* running_var, float* y, float* save_mean, float* save_invstd, int B, int C, int L,
                  float eps, float momentum, int training, int act, float slope, const float* residual, void* ws,
                  size_t ws_bytes, void* scratch, long long y_batch_stride, void* stream);
int m2d_bn_fwd_sums_to(const float* x, const double* sums, double count, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, float* y, float* save_mean, float* save_invstd, int B,
                       int C, int L, float eps, float momentum, int act, float slope, const float* residual,
                       long long y_batch_stride, void* stream);
/* Round 6: m2d_bn_fwd_sums_to with the pass that follows it in the U-Net fused in (phase3/archis/default.py:235-245):
 * MaxPool1d(2, 2) behind a skip's BatchNorm (y AND pooled (B, C, L / 2) are written; L even), Upsample(scale_factor=2, linear)
 * behind a decoder level's (only the upsampled (B, C, 2L) tensor is written, at up + b * up_batch_stride; C * L even). Same
 * values, save_* and running buffers as m2d_bn_fwd_sums_to followed by m2d_maxpool2_fwd_from / m2d_upsample2_fwd_to. */
int m2d_bn_fwd_sums_pool_to(const float* x, const double* sums, double count, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, float* y, float* pooled, float* save_mean,
                            float* save_invstd, int B, int C, int L, float eps, float momentum, int act, float slope,
                            long long y_batch_stride, void* stream);
int m2d_bn_fwd_sums_upsample2_to(const float* x, const double* sums, double count, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var, float* up, float* save_mean, float* save_invstd,
                                 int B, int C, int L, float eps, float momentum, int act, float slope,
                                 long long up_batch_stride, void* stream);
int m2d_bn_bwd_stats(const float* dy, const float* x, const float* gamma, const float* beta, const float* save_mean,
                     const float* save_invstd, double* sums, int B, int C, int L, int act, float slope,
                     void* scratch, void* stream);
int m2d_bn_bwd_sums(const float* dy, const float* x, const float* gamma, const float* beta, const float* save_mean,
                    const float* save_invstd, const double* sums_local, const double* sums_global, double count,
                    float* dx, float* dgamma, float* dbeta, int B, int C, int L, int act, float slope, void* ws,
                    size_t ws_bytes, void* stream);
int m2d_channel_sums(const float* x, const float* mask, float slope, float* out, int B, int C, int L, void* ws,
                     size_t ws_bytes, void* scratch, void* stream);

/* ---- GRU recurrence (one layer, all T steps) ---------------------------------------------
 * reference: nn.GRU inside NoiseGen, phase3/archis/default.py:349-355,
 * phase2/archis/default.py:90-96. gi = x W_ih^T + b_ih is an m2d_gemm (mode 0). */
int m2d_gru_layer_fwd(const float* gi, const float* w_hh_t, const float* b_hh, const int* lengths, float* out,
                      float* r_s, float* z_s, float* n_s, float* hn_s, int B, int T, int H, void* stream);
int m2d_gru_layer_bwd(const float* dout, const float* out, const float* r_s, const float* z_s, const float* n_s,
                      const float* hn_s, const float* w_hh, const int* lengths, float* dgi, float* dgh,
                      float* dh_buf, int B, int T, int H, void* stream);

/* Whole L-layer stack (L <= 4, equal hidden sizes) on the (layer, t) diagonal: T + L - 1 launches
 * instead of L * T. Pointer arrays have L entries; w_ih_t[0] / b_ih[0] / w_ih[0] are ignored (layer 0's
 * projection gi0 comes from m2d_gemm). saved[l]: (4, B, T, H) = r, z, n, W_hn h + b_hn (or saved == NULL). */
/* `counters` (optional): m2d_gru_stack_counters(B, L) unsigneds of device scratch owned by this call. With it, and
 * when every (layer, batch tile, hidden tile) workgroup fits on the chip at once, the whole recurrence runs as ONE
 * persistent launch (weight slices resident in LDS, per-step hand-off between CUs through write-through stores
 * and agent-scope counters); results are bit-identical to the per-step launches. Spins are bounded: a timeout
 * raises a flag readable through m2d_gru_persist_error() after a stream synchronisation (outputs then invalid).
 * M2D_PERSISTENT_GRU=0 disables the persistent form (needed when several processes share one GPU: their
 * persistent kernels could starve each other of CUs). */
int m2d_gru_stack_counters(int B, int L);
int m2d_gru_stack_fwd(const float* gi0, const float* const* w_ih_t, const float* const* b_ih,
                      const float* const* w_hh_t, const float* const* b_hh, float* const* out, float* const* saved,
                      const int* lengths, int B, int T, int H, int L, unsigned* counters, void* stream);
/* m2d_gru_stack_fwd with a carried recurrent state (inference: no backward through h0). h0 (L entries) or NULL:
 * h0[l] (B, H) is layer l's state before step 0 (a NULL entry: zeros, bit-identical to m2d_gru_stack_fwd); step 0
 * then computes the full W_hh h0 + b_hh product, in both the per-step and the persistent form. h_n (L entries) or
 * NULL: h_n[l] (B, H) receives the state after step lengths[b] - 1 (T - 1 without lengths) - torch's h_n. A sequence
 * split in two calls chained through h_n -> h0 gives the bits of one call over the whole sequence. */
int m2d_gru_stack_fwd_state(const float* gi0, const float* const* w_ih_t, const float* const* b_ih,
                            const float* const* w_hh_t, const float* const* b_hh, float* const* out,
                            float* const* saved, const int* lengths, const float* const* h0, float* const* h_n, int B,
                            int T, int H, int L, unsigned* counters, void* stream);
int m2d_gru_persist_error(void);
/* Recovery from such a timeout without leaving the process: m2d_gru_persist_peek() reads the word without clearing it,
 * m2d_async_fault_word() is the address of its device-memory copy (or NULL; a timed-out launch raises both) - passed to m2d_adam_multi as `skip`, every optimizer
 * step queued behind the failed recurrence voids itself on the device; the host then synchronises, clears the word
 * (m2d_gru_persist_error) and carries on with the per-step launches (engine.py). m2d_gru_persist_raise(): test hook. */
int m2d_gru_persist_peek(void);
void* m2d_async_fault_word(void);
int m2d_gru_persist_raise(void);
/* dst[0] (device float) = 1.0 when the word is raised, else 0.0: what a data-parallel gradient exchange adds to its last
 * bucket so that every rank skips the optimizer steps one rank has to skip (dp.GradExchange.fault_flag). */
int m2d_fault_fetch(float* dst, void* stream);
int m2d_gru_stack_bwd(const float* dout, const float* const* out, const float* const* saved,
                      const float* const* w_hh, const float* const* w_ih, float* const* dgi, float* const* dgh,
                      float* const* dh_buf, const int* lengths, int B, int T, int H, int L, unsigned* counters,
                      void* stream);
/* `counters` of m2d_gru_stack_bwd (optional, m2d_gru_stack_counters(B, L) unsigneds of scratch owned by the call): with
 * them the whole back-propagation through time runs as ONE persistent launch too (round 3): weight slices in LDS,
 * dgh_l[t+1] / dgi_{l+1}[t] handed over between CUs inside the launch; bit-identical to the per-step launches. */

/* ---- small-state GRU (1 <= H <= 16; H outside gives M2D_ERR_ARG) --------------------------
 * reference: nn.GRU(128, 4) of RecurrentDanceClassifier, dance_classification/archis/default.py:18,24, whose
 * final state h_n is the logits. One layer, the whole sequence in ONE launch: one batch row per 16-lane group,
 * W_hh / b_hh in registers, h broadcast inside the group. gi = x W_ih^T + b_ih comes from m2d_gemm (mode 0);
 * w_hh is (3H, H) as nn.GRU stores it. out (B, T, H) or NULL: rows past lengths[b] are 0, as in
 * m2d_gru_layer_fwd. h_n (B, H): the state after step lengths[b] - 1 (T - 1 without lengths) - torch's h_n.
 * saved (4, B, T, H) or NULL: r, z, n, W_hn h + b_hn (the layout of m2d_gru_stack_fwd).
 * The backward (BPTT, one launch) takes dout (B, T, H) and / or dh_n (B, H) (either may be NULL), the forward's
 * out (required: it holds h_{t-1}) and saved state, and writes dgi and dgh (B, T, 3H) with the contract of
 * m2d_gru_layer_bwd: weight, bias and input gradients then come from m2d_gemm modes 1 / 2 and m2d_channel_sums. */
int m2d_gru_small_fwd(const float* gi, const float* w_hh, const float* b_hh, const int* lengths, float* out,
                      float* h_n, float* saved, int B, int T, int H, void* stream);
int m2d_gru_small_bwd(const float* dout, const float* dh_n, const float* out, const float* saved, const float* w_hh,
                      const int* lengths, float* dgi, float* dgh, int B, int T, int H, void* stream);

/* ---- softmax cross-entropy (torch.nn.CrossEntropyLoss, mean; dance_classification/main.py:126) ----------
 * logits (B, C), C <= 1024 (M2D_ERR_ARG beyond); labels int64 (B); loss: one float (0-dim). Max-subtracted
 * log-sum-exp per row, the per-row losses summed in fp64 in a fixed order (bit-stable from run to run).
 * pred (int64 (B) or NULL): the argmax, first maximum on ties (torch.argmax). A label outside [0, C) makes the
 * loss (and that row's gradient) NaN; nothing asserts on the device. ws: m2d_cross_entropy_workspace_bytes.
 * The backward writes dlogits = (softmax - onehot) * gout[0] / B, gout a device scalar. */
size_t m2d_cross_entropy_workspace_bytes(int B, int C);
int m2d_cross_entropy_fwd(const float* logits, const long long* labels, float* loss, long long* pred, int B, int C,
                          void* ws, size_t ws_bytes, void* stream);
int m2d_cross_entropy_bwd(const float* logits, const long long* labels, const float* gout, float* dlogits, int B,
                          int C, void* stream);

/* ---- binary cross-entropy on logits (torch.nn.BCEWithLogitsLoss, mean; phase2/train.py:204-240, `-f gan`) --------
 * BCEWithLogitsLoss(reduction='mean') per segment: x = (n0 + n1) logits, segment 0 against target t0, segment 1
 * (n1 may be 0) against t1. out[0] = mean_0 + mean_1, out[1] = mean_0, out[2] = mean_1 (0 when n1 == 0).
 * dx (optional, NULL = not written) = d out[0] / dx = (sigmoid(x) - t) / n_segment.
 * Elements as torch computes them, max(x, 0) - x t + log1p(exp(-|x|)), in fp64; each segment summed in fp64 in a
 * fixed order by one workgroup (bit-stable from run to run). A NaN logit gives a NaN loss and gradient.
 * n0 <= 0 or n1 < 0: M2D_ERR_ARG. */
int m2d_bce_logits_fwd(const float* x, int n0, float t0, int n1, float t1, float* out, float* dx, void* stream);
/* dx = gout[0] * (sigmoid(x) - t) / n_segment, gout a device scalar */
int m2d_bce_logits_bwd(const float* x, int n0, float t0, int n1, float t1, const float* gout, float* dx,
                       void* stream);

/* ---- gradient penalty (losses.py:5-60) ----------------------------------------------------- */
int m2d_gp_interpolate(const float* real, const float* fake, const float* alpha, float* out, int B, int n,
                       void* stream);
size_t m2d_gp_penalty_workspace_bytes(int B);
int m2d_gp_penalty_fwd(const float* g, float* norms, float* penalty, int B, int n, int lp, void* ws, size_t ws_bytes,
                       void* stream);
int m2d_gp_penalty_bwd(const float* g, const float* norms, const float* gout, float* dg, int B, int n, int lp,
                       void* stream);

/* ---- L1 / total-variation losses (phase3/train.py:170,226; losses.py:76-82) ---------------- */
size_t m2d_reduce_workspace_bytes(void);
int m2d_l1_mean_fwd(const float* a, const float* b, float* out, size_t n, void* ws, size_t ws_bytes, void* stream);
int m2d_l1_mean_bwd(const float* a, const float* b, const float* gout, float* da, size_t n, void* stream);
int m2d_tv_mean_fwd(const float* x, float* out, int B, int C, int T, long sb, long sc, long st, void* ws,
                    size_t ws_bytes, void* stream);
int m2d_tv_mean_bwd(const float* x, const float* gout, float* dx, int B, int C, int T, long sb, long sc, long st,
                    void* stream);

/* ---- evaluation metric + dataset scaling ------------------------------
 * m2d_jerk_mean_fwd: losses.py:85-89 `jerkiness` (phase3/test.py:78-104) on a (B, C, T) tensor given by element
 *   strides: sum over channels of the squared third time difference, mean over (B, T-3).
 * m2d_affine_cols: y[r, c] = x[r, c] * scale[c] + shift[c]: sklearn MinMaxScaler.transform (scale_, min_) /
 *   inverse_transform (1/scale_, -min_/scale_) as the reference's datasets apply it (utils.py:26-31,79-85;
 *   phase2/train.py:192-193). y may alias x. */
int m2d_jerk_mean_fwd(const float* x, float* out, int B, int C, int T, long sb, long sc, long st, void* ws,
                      size_t ws_bytes, void* stream);
int m2d_affine_cols(const float* x, const float* scale, const float* shift, float* y, size_t rows, int cols,
                    void* stream);

/* ---- optimizer step (phase3/train.py:102-103,214,238; phase2/train.py:86-87; phase1/train_wgan-gp.py:60-61) ----
 * torch.optim.Adam(params, lr) with its defaults (betas 0.9 / 0.999, eps 1e-8, no weight decay, no amsgrad) over
 * MANY tensors in one launch (per 48 tensors), optionally writing a conv weight's two K-major packed images
 * (m2d_conv1d_pack_weights) in the same pass - the critic's weights change every loop body, and their images with them:
 *   m = m + (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g g;
 *   p = p - (lr / bias_corr1) m / (sqrt(v) / bias_corr2_sqrt + eps)
 * with bias_corr1 = 1 - beta1^step, bias_corr2_sqrt = sqrt(1 - beta2^step) computed by the caller (the arithmetic of
 * torch's fused implementation). `items`: HOST array of n records; tensors whose gradient is absent are simply not
 * listed (torch skips them). pack_fwd / pack_bwd (either may be NULL) only for 3-D conv weights
 * (cout, cin, ks). `skip` (optional): device-visible 32-bit word; when any of its bits is set at execution time the whole step is a no-op -
 * the hook by which a failed launch upstream (a persistent recurrent kernel that timed out) voids the update on
 * the device, without a host round trip. */
typedef struct M2dAdamItem {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  long long numel;
  float* pack_fwd;   /* (cin, ks, cout) image or NULL */
  float* pack_bwd;   /* (cout, ks, cin) image or NULL */
  int cout, cin, ks, reserved;
} M2dAdamItem;
int m2d_adam_multi(const M2dAdamItem* items, int n, float lr, float beta1, float beta2, float eps, float bias_corr1,
                   float bias_corr2_sqrt, const float* skip, void* stream);
/* The same step with an exponential moving average of the parameters kept in the same launch (40 tensors per launch):
 * `ema` is a HOST array of n device pointers, ema[i] the shadow of items[i].param (same element count) or NULL for a
 * tensor stepped without one; a NULL `ema` with n > 0 is M2D_ERR_ARG. After p has been updated exactly as above
 * (p, exp_avg, exp_avg_sq and both packed images are bit-identical to m2d_adam_multi's), per element and in fp32, from
 * the register copy of the fresh p:
 *   e = e + ema_one_minus_decay * (p - e)
 * The shadow's alignment counts with the other pointers' (a shadow off 16 bytes is never read as a vector). `skip`
 * voids the shadows' update with the step. */
int m2d_adam_multi_ema(const M2dAdamItem* items, float* const* ema, int n, float lr, float beta1, float beta2,
                       float eps, float bias_corr1, float bias_corr2_sqrt, float ema_one_minus_decay,
                       const float* skip, void* stream);

/* ---- U-Net encoder resampling (phase3/archis/default.py:235-245) --------------------------- */
int m2d_maxpool2_fwd(const float* x, float* y, size_t rows, int L, void* stream);
int m2d_maxpool2_bwd(const float* x, const float* dy, float* dx, size_t rows, int L, void* stream);
int m2d_upsample2_fwd(const float* x, float* y, size_t rows, int L, void* stream);
int m2d_upsample2_fwd_to(const float* x, float* y, size_t B, int C, int L, long long y_batch_stride, void* stream);
int m2d_maxpool2_fwd_from(const float* x, float* y, size_t B, int C, int L, long long x_batch_stride, void* stream);
int m2d_upsample2_bwd(const float* dy, float* dx, size_t rows, int L, void* stream);

/* ---- label conditioning and dropout of the conditional phase-2 networks (phase2/archis/conditional.py) ---------- */
/* out = [x | E[labels[b]]] for every (b, t). layout 0 (batch-first): x (B, T, C), out (B, T, C + D); layout 1
   (channels-first): x (B, C, T), out (B, C + D, T). E (L, D); labels int64 (B,). A label outside [0, L) makes the D
   label features of its row NaN (nothing is read out of bounds). */
int m2d_label_concat(const float* x, const float* E, const long long* labels, float* out, int B, int T, int C, int L,
                     int D, int layout, void* stream);
/* m2d_pose_pack3 with label channels: out (3B, C + D, T) = [interpolated | real | fake] channels-first; the interpolated
   and real rows carry E[real_lbl[b]], the fake rows E[fake_lbl[b]], constant over time */
int m2d_pose_pack3_label(const float* real, const float* fake, const float* alpha, const float* E,
                         const long long* real_lbl, const long long* fake_lbl, float* out, int B, int T, int C, int L,
                         int D, void* stream);
/* dE[l, d] = sum over rows r in [r0, r1) with labels[r - r0] == l of sum_t dx[r, c0 + d, t] (layout 0: dx (R, T, Ctot),
   layout 1: dx (R, Ctot, T)); dE (L, D) is overwritten. One workgroup per (l, d), fixed-order fp64 sum, no atomics:
   bit-stable. Any label of the range outside [0, L): every dE entry is NaN. */
int m2d_label_embed_bwd(const float* dx, const long long* labels, float* dE, int r0, int r1, int T, int Ctot, int c0,
                        int L, int D, int layout, void* stream);
/* y = x * keep * scale over n elements. gen = 0: keep = mask[i] != 0 (bytes). gen = 1: keep = (u >> 8) * 2^-24 < p_keep
   with u word i % 4 of Philox4x32-10(counter = (i / 4, offset), key = seed); mask (optional) receives the keep bytes.
   x = NULL: the mask only (gen = 1). */
int m2d_dropout(const float* x, float* y, unsigned char* mask, long long n, float p_keep, float scale,
                unsigned long long seed, unsigned long long offset, int gen, void* stream);
/* out (B, n, C) = standard normals; the value of (b, frame0 + i, c) is a pure function of (seed, b, frame0 + i, c):
   Philox4x32-10(counter = (c / 4, frame as 64 bits, b), key = seed) followed by Box-Muller. A track's noise is then
   the same whatever chunks its frames are generated in. */
int m2d_randn_frames(float* out, unsigned long long seed, long long frame0, int B, int n, int C, void* stream);

/* ---- stick-figure video frames (visualize.py:195-255: draw, frame_to_vid) ------------------------------------------
 * poses (n_frames, 69) fp32, world coordinates (joint j = (x, y, z) at 3j..3j+2; z unused) -> out (n_frames, height,
 * width, 3) uint8 RGB, every byte written: white, with 23 disks (radius 4) and 21 segments (width 3) in blue
 * (0, 0, 255), the reference's skeleton. x' = fl32(x + width/2), y' = fl32(y + height/2); pixel (trunc(x'), trunc(y')),
 * a midpoint trunc(fl32(fl32(a' + b') * 0.5)); image row = height - 1 - pixel height. A joint with a non-finite
 * coordinate or |x'| or |y'| >= 2^14 draws nothing, nor does any segment that uses it. Coverage is exact in integers:
 * a disk covers (c - px)^2 + (r - py)^2 <= 16, a segment the pixels at squared distance <= 1.
 * height, width in [1, 4096]; n_frames 0: nothing to do. Deterministic, no atomics. */
int m2d_render_sticks(const float* poses, long n_frames, int height, int width, unsigned char* out, void* stream);
/* Baseline JPEG streams of frames (n_frames, height, width, 3) uint8 RGB on the device (contiguous, any byte
 * alignment), one complete stream per frame: JFIF, 8 bits, 4:4:4, one interleaved scan, the standard's typical Huffman
 * tables, a restart interval of one row of 8 x 8 blocks; integer colour transform, DCT and quantisation, stated in
 * numpy by tests/jpeg_rule.py, which the bytes equal. qtabs: HOST memory, 128 bytes, the
 * luminance then the chrominance quantisation table in row-major order, entries 1..255 (read before the call returns).
 * out: device buffer of `capacity` bytes that receives the streams back to back; offsets: n_frames + 1 int64 on the
 * device, frame i occupies out[offsets[i], offsets[i + 1]). offsets are always written. If offsets[n_frames] > capacity
 * nothing is written to out (no truncation): call again with that capacity. Never writes out of [0, offsets[n_frames])
 * nor past capacity. workspace: m2d_jpeg_workspace_bytes(n_frames, height, width) bytes, 16-byte aligned (int16
 * coefficients of every block, row and frame sizes). Five launches on `stream`; deterministic, no host
 * synchronisation, no allocation, capturable. height, width in [1, 4096]; n_frames 0: nothing to do.
 * M2D_ERR_ARG: sizes out of range, a null pointer, a zero table entry; M2D_ERR_WORKSPACE; M2D_ERR_RANGE: more rows of
 * blocks than one launch takes. */
size_t m2d_jpeg_workspace_bytes(long n_frames, int height, int width);
int m2d_jpeg_encode(const unsigned char* frames, long n_frames, int height, int width, const unsigned char* qtabs,
                    unsigned char* out, long long capacity, long long* offsets, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- polyphase FIR resampling of audio rows (change_rate.py:6-8: the reference shells out to sox) -----------------
 * Row b of x (B rows, ldx floats apart) holds the samples with ABSOLUTE indices [x0, x0 + nx); every other sample is
 * zero. half = (ntaps - 1) / 2 (ntaps odd, <= 16384). For output index n in [n0, n0 + ny), with t = n down + half:
 *   y[b ldy + n - n0] = sum over all integers m with 0 <= t - m up < ntaps of taps[t - m up] X_b[m]
 * = scipy.signal.resample_poly(x, up, down, window=taps / up, padtype='constant'): zero phase, output n sits at input
 * time n down / up. up / down must be reduced by their gcd. All index arithmetic is 64-bit (n down may pass 2^32;
 * n down + half must stay below 2^63). The value of output n is a bit-level pure function of n, the taps and the
 * samples of its window - one fp32 accumulator, fmaf over its taps in ascending tap index (descending m) - and does not
 * depend on n0, x0, ny, nx, the launch's tiling or B: the chunks of a stream equal the whole-track call bit for bit.
 * M2D_ERR_ARG (nothing launched): up, down or B <= 0; nx, ny, x0 or n0 < 0; even ntaps or ntaps > 16384; ldx < nx or
 * ldy < ny; an unreduced ratio. ny == 0: nothing to do. */
int m2d_resample_poly(const float* x, long long x0, int nx, long long ldx, const float* taps, int ntaps, int up,
                      int down, float* y, long long n0, int ny, long long ldy, int B, void* stream);

/* ---- crop + augment gather of a training batch (data.py: SequenceDataset.sample_batch; the
 * reference augments on disk, augment_data.py) ------------------------------------------------------------------------
 * poses (frames, C) fp32: the takes of the dataset back to back, C a multiple of 3 (joint j = columns 3j .. 3j + 2 =
 * x, y, z; y is the vertical axis). track (samples) fp32: their audio tracks back to back, or NULL with S == 0 (the
 * audio-less loaders). rows: DEVICE array of B records, filled by the host:
 *   pose_start              row of the store that output frame 0 shows; pose_first / pose_last: the first and the last
 *                           row of the row's own take (inclusive)
 *   audio_start             sample of the store that output sample 0 sits on; audio_first / audio_last: the first and
 *                           the last sample of the row's own take (inclusive)
 *   a, b                    playback speed a / b, reduced, 1 <= a, b <= 64
 *   tap_offset, ntaps       the row's filter taps[tap_offset .. tap_offset + ntaps) in the concatenated tap buffer
 *                           (ntaps odd, <= 1281; not read at speed 1/1)
 *   mirror, cos_yaw, sin_yaw, gain
 * out_poses (B, T, C): frame i of row r shows source position pose_start + i a / b: j = (i a) div b, f = ((i a) mod b) /
 *   b; v = x[j] when f == 0, else fmaf(f, x[j + 1] - x[j], x[j]) (j + 1 clamped to pose_last, read only when f != 0).
 *   With mirror == 0, cos_yaw == 1 and sin_yaw == 0 the output is v. Otherwise per joint, with u = (v - shift[col]) /
 *   scale[col]: ux = -ux under mirror; x' = fmaf(c, ux, s uz), z' = fmaf(c, uz, -(s ux)), y' = uy; out = fmaf(u',
 *   scale[col], shift[col]). scale, shift: C floats each.
 * out_audio (B, S): m2d_resample_poly's formula with up = b, down = a on X[m] = track[audio_start + m] where that
 *   index lies in [audio_first, audio_last], zero elsewhere: t = n a + half, half = (ntaps - 1) / 2,
 *   y[n] = gain * sum over m with 0 <= t - m b < ntaps of taps[t - m b] X[m] - one fp32 accumulator, fmaf in ascending
 *   tap index, then one multiply by gain: with gain == 1 the bits of m2d_resample_poly on the take alone. Speed 1/1:
 *   y[n] = gain X[n].
 * All source indexing is 64-bit; every read lies inside the row's own take (and inside the store, whatever the table
 * says). One launch on `stream`, no workspace, no atomics: an output element is a bit-level pure function of its row's
 * record and its index, whatever B, the row's position and the launch's tiling. A record the Python wrapper would have
 * refused (a or b outside [1, 64], bad taps) gives NaN, never a stray read.
 * M2D_ERR_ARG (nothing launched): B, T or C <= 0; S < 0; C % 3 != 0; a null pose store, table, scale, shift or
 * out_poses, or frames <= 0; S > 0 with a null track store, taps or out_audio, or samples or taps_total <= 0. */
typedef struct M2dAugmentRow {
  long long pose_start, pose_first, pose_last;
  long long audio_start, audio_first, audio_last;
  int a, b, tap_offset, ntaps, mirror;
  float cos_yaw, sin_yaw, gain;
} M2dAugmentRow;
int m2d_crop_augment(const float* poses, long long frames, int C, const float* track, long long samples,
                     const M2dAugmentRow* rows, const float* scale, const float* shift, const float* taps,
                     int taps_total, float* out_poses, float* out_audio, int B, int T, int S, void* stream);

/* ---- beat alignment of a dance with its music (metrics.py; no counterpart in the reference) --
 * STFT band energies. n_fft: a power of two in [256, 2048]; nbins = n_fft / 2 + 1; w[n] = 0.5 - 0.5 cos(2 pi n / n_fft)
 * (periodic Hann). Row b of x (B rows, ldx floats apart) holds samples [0, S) of a track, every other sample is zero.
 * Frame t (any t >= 0, 64-bit) starts at sample s_t = t hop + hop / 2 - n_fft / 2 (integer divisions). For frames
 * t = frame0 .. frame0 + T - 1 and bands 0 .. nb - 1 (nb <= 128):
 *   re[k] = sum_n table[0][k][n] x[s_t + n], im[k] = sum_n table[1][k][n] x[s_t + n], P[k] = re^2 + im^2 (k < nbins),
 *   E[(b T + t - frame0) nb + band] = sum_k bands[band nbins + k] P[k]
 * with table (2, nbins, n_fft) = [w[n] cos(2 pi ((n k) mod n_fft) / n_fft); -w[n] sin(the same)], made on the HOST in
 * fp64 and rounded to fp32 (the device never takes the cosine of a large argument). The kernel reads the table as the
 * packed image pack_basis makes of it (image_elems floats, 16-byte aligned; image_elems is 0 for a bad n_fft): the
 * sine row of bin 0 is identically zero and is not kept, its place carries the cosine row of bin n_fft / 2. All sums
 * are fp32 (v_mfma_f32_32x32x2_f32 for both contractions) in a fixed order: the value of a frame is a bit-level pure
 * function of t, the samples of its window, the table and the bands, whatever frame0, T, B, ldx and the launch's
 * tiling - a track may be processed in chunks of frames. Frames that lie past the track are exactly zero. No atomics,
 * no workspace; neither the windows (B, T, n_fft) nor the spectrum (B, T, 2 nbins) is ever written.
 * M2D_ERR_ARG (nothing launched): n_fft not such a power of two; nb outside [1, 128]; hop or B <= 0; T, S or frame0
 * < 0; ldx < S; a null or misaligned pointer; (frame0 + T) hop near 2^63. T == 0: nothing to do. */
size_t m2d_stft_image_elems(int n_fft);
int m2d_stft_pack_basis(const float* table, int n_fft, float* image, void* stream);
int m2d_stft_bands(const float* x, long long ldx, int S, int B, long long frame0, int T, int hop, int n_fft,
                   const float* image, const float* bands, int nb, float* E, void* stream);
/* onset strength of band energies E (B, T, nb), contiguous: o[b T] = 0 and, for t >= 1,
 *   o[b T + t] = (1 / nb) sum_band max(0, log1pf(gamma E[t][band]) - log1pf(gamma E[t - 1][band])),
 * one fp32 accumulator over ascending bands. gamma >= 0. One pass, no workspace. */
int m2d_onset_flux(const float* E, int B, int T, int nb, float gamma, float* o, void* stream);
/* mean joint speed of poses (B, T, J, 3), contiguous, T >= 2: for t >= 1
 *   v[b T + t] = (1 / J) sum_j sqrtf(dx^2 + dy^2 + dz^2), d = p[t][j] - p[t - 1][j],
 * one fp32 accumulator over ascending j; v[b T] = v[b T + 1] (the same operations). */
int m2d_motion_speed(const float* poses, int B, int T, int J, float* v, void* stream);
/* Beat alignment of onset strength o and motion speed v, both (B, T) contiguous, row by row (one workgroup a row):
 *   smoothing g(c, sigma)[t] = sum_j w_j c[t + j] / sum_j w_j over j in [-R, R] with 0 <= t + j < T, R = ceil(3 sigma),
 *     w_j = exp(-j^2 / (2 sigma^2)): summed in fp64 in ascending j and rounded to fp32 once;
 *   music events M: t in [1, T - 2] with s[t] > s[t - 1], s[t] >= s[t + 1] and s[t] > mean_t s, s = g(o, sigma_onset);
 *   motion events K: t in [1, T - 2] with u[t] < u[t - 1] and u[t] <= u[t + 1], u = g(v, sigma_speed);
 *   scores[4 b + 0] = mean over k in K of expf(-d^2 / (2 sigma_align^2)), d = min over m in M of |k - m|
 *     (two directional scans), [4 b + 1] the same with K and M exchanged, [4 b + 2] = |K|, [4 b + 3] = |M|;
 *     both scores are NaN when K or M is empty (always for T < 3).
 * Optional outputs (NULL: not wanted): motion_events, music_events (B, T) bytes 0 / 1; onset_smooth, speed_smooth
 * (B, T) fp32. Every sum has a fixed order, no atomics: bit-stable. M2D_ERR_ARG (nothing launched): B <= 0, T < 0,
 * T > max_frames (16384), a sigma <= 0 or a radius ceil(3 sigma) > 64, a null pointer. */
int m2d_beat_align_max_frames(void);
int m2d_beat_align(const float* onset, const float* speed, int B, int T, double sigma_onset, double sigma_speed,
                   double sigma_align, float* scores, unsigned char* motion_events, unsigned char* music_events,
                   float* onset_smooth, float* speed_smooth, void* stream);

/* ---- distribution scores of a set of dances (metrics.py; no counterpart in the reference) ------
 * Here `mean`, `cov`, the matrices, eigenvalues and scores are DOUBLE; every sum has a fixed order (no atomics): results
 * are bit-identical from run to run. A null or a host pointer is refused (M2D_ERR_ARG, nothing launched).
 *
 * Kinetic features of poses (B, T, J, 3), contiguous, T >= 3, fps > 0, up_axis in 0..2. With d[t] = p[t] - p[t - 1]
 * (taken in fp32), v[t] = d[t] fps and a[t] = (d[t + 1] - d[t]) fps^2 (the second difference, also fp32), joint j gives
 *   F[b][j]         = mean over t = 1 .. T - 1 of v[t][o1]^2 + v[t][o2]^2  (o1 < o2 the axes other than up_axis),
 *   F[b][J + j]     = mean over t = 1 .. T - 1 of v[t][up_axis]^2,
 *   F[b][2 J + j]   = mean over t = 1 .. T - 2 of sqrt((a[t][o1]^2 + a[t][o2]^2) + a[t][up_axis]^2),
 * products and sums in fp64 (256 interleaved partial sums, then a tree), rounded to fp32 once. One workgroup per (b, j):
 * row b does not depend on B. M2D_ERR_ARG: B or J <= 0, T < 3, fps <= 0, up_axis outside 0..2. */
int m2d_kinetic_features(const float* poses, int B, int T, int J, double fps, int up_axis, float* F, void* stream);
/* the largest order m2d_sym_eig, m2d_feature_moments and m2d_frechet take (128), and the sweep cap of the solver (30) */
int m2d_sym_eig_max_dim(void);
int m2d_sym_eig_max_sweeps(void);
/* mean (D) and unbiased covariance (D, D) of the rows of X (N, D) fp32, rows ldx floats apart: two passes,
 *   mean[d] = (1 / N) sum_n x[n][d],  cov[i][j] = (1 / (N - 1)) sum_n (x[n][i] - mean[i]) (x[n][j] - mean[j]),
 * every operation fp64 (the second sum in ascending n with fma): cov is exactly symmetric.
 * M2D_ERR_ARG: N < 2, D outside [1, max_dim], ldx < D. */
int m2d_feature_moments(const float* X, long long ldx, int N, int D, double* mean, double* cov, void* stream);
/* Eigenvalues w (P, D), ascending, of P symmetric matrices A (P, D, D) (the whole matrix is read), and with vecs != NULL
 * the eigenvectors as the COLUMNS of vecs (P, D, D): A vecs[:, i] = w[i] vecs[:, i]. Two-sided cyclic Jacobi in a
 * round-robin ordering, one workgroup per matrix, the matrix in LDS. info (P, 2): [sweeps used, converged (1 / 0)].
 * Converged: the squared off-diagonal norm a sweep met is at most (2^-50 ||A||_F)^2. At most max_sweeps sweeps run
 * whatever the data; a matrix that holds a NaN or an infinity runs all of them and gives NaN eigenvalues (and vectors)
 * with converged = 0. Squares of the entries must be representable. Workspace: only with vecs.
 * M2D_ERR_ARG: P <= 0, D outside [1, max_dim]; M2D_ERR_WORKSPACE: ws too small. */
size_t m2d_sym_eig_workspace_bytes(int P, int D, int vectors);
int m2d_sym_eig(const double* A, int P, int D, double* w, double* vecs, double* info, void* ws, size_t ws_bytes,
                void* stream);
/* Frechet distance of P pairs of Gaussians: mean1, mean2 (P, D), cov1, cov2 (P, D, D) -> out (P, 6):
 *   [fd, |mean1 - mean2|^2, tr cov1 + tr cov2, tr (cov1 cov2)^1/2, sweeps (the larger of the two solves), converged],
 *   fd = (|mean1 - mean2|^2 + tr cov1 + tr cov2) - 2 tr (cov1 cov2)^1/2, NOT clipped at zero;
 *   tr (cov1 cov2)^1/2 = sum_i sqrt(max(l_i, 0)), l the eigenvalues of cov1^1/2 cov2 cov1^1/2, taken in the eigenbasis
 *   of cov1 = V L V^T, where that matrix is max(L, 0)^1/2 (V^T cov2 V) max(L, 0)^1/2.
 * Five launches on `stream` (m2d_sym_eig's kernel twice, two products, the sums), no host synchronisation, no other
 * library. M2D_ERR_ARG: P outside [1, 65535], D outside [1, max_dim]; M2D_ERR_WORKSPACE: ws too small. */
size_t m2d_frechet_workspace_bytes(int P, int D);
int m2d_frechet(const double* mean1, const double* cov1, const double* mean2, const double* cov2, int P, int D,
                double* out, void* ws, size_t ws_bytes, void* stream);
/* X (G K, D) fp32, rows ldx floats apart, G groups of K consecutive rows -> out[g] = the mean over the K (K - 1) / 2 pairs
 * i < j of group g of sqrt(sum_d (x_i[d] - x_j[d])^2): the difference in fp32, squares and sums in fp64 (ascending d; the
 * pairs of a row i over 256 interleaved partial sums and a tree, then the rows likewise). K = 1: NaN. A group's value
 * does not depend on G. M2D_ERR_ARG: G, K or D <= 0, G > 65535, ldx < D; M2D_ERR_WORKSPACE: ws too small. */
size_t m2d_pairwise_mean_dist_workspace_bytes(int G, int K);
int m2d_pairwise_mean_dist(const float* X, long long ldx, int G, int K, int D, double* out, void* ws, size_t ws_bytes,
                           void* stream);

/* ---- audio-motion synchronisation of a take (metrics.py; no counterpart in the reference) ----
 * out[b T + t] = g(c[b], sigma)[t], the smoothing of m2d_beat_align (the same device function: bit-equal to its
 * onset_smooth / speed_smooth for the same row and sigma), for c (B, T) contiguous of ANY length T >= 0.
 * M2D_ERR_ARG (nothing launched): B <= 0, T < 0, sigma <= 0 or ceil(3 sigma) > 64, a null pointer. */
int m2d_gauss_smooth(const float* c, int B, int T, double sigma, float* out, void* stream);
/* Lag / tempo-factor profile. a (B, Ta) and b (B, Tb) fp32, rows lda / ldb floats apart; na_rows / nb_rows: optional
 * DEVICE int32 (B) lengths of the rows (NULL: Ta / Tb for every row). For row b with na frames of a and nb of b, factor
 * f = factors[i] (F HOST doubles) and integer lag l in [-L, L], take every j in [0, na) with x = (double)(j + l) / f in
 * [0, nb - 1] and pair a[j] with bv = b[i] + fr (b[min(i + 1, nb - 1)] - b[i]), i = floor(x), fr = x - i, in fp64
 * from the fp32 values (f == 1: b[j + l] exactly). n = the number of pairs;
 *   r = S_ab / sqrt(S_aa S_bb), two passes in fp64: the means of the pairs, then the sums of the centred products;
 *   r = NaN when n < min_overlap or S_aa or S_bb is 0. l > 0: the motion (b) lags the audio (a) by l frames.
 * r (B, F, 2 L + 1) double and n (B, F, 2 L + 1) int32, lag l at index l + L. One wave a cell: lane k sums the j = k
 * (mod 64) in ascending j, the 64 partials are added by the butterfly 32, 16, .., 1: r and n are bit-level pure
 * functions of the row's values, na, nb, f, l and min_overlap - not of B, F, L, the strides or the launch. No atomics,
 * no workspace. A length of 0 gives NaN and n = 0.
 * M2D_ERR_ARG (nothing launched): B or F <= 0; L < 0; a factor not finite or <= 0; min_overlap < 2; Ta or Tb < 0 or
 * above max_frames (16384); a row length outside [0, T] (read back with one small copy, except inside a stream capture,
 * where such a row counts as empty); lda < Ta or ldb < Tb; a null or misaligned pointer. */
int m2d_sync_scan_max_frames(void);
int m2d_sync_scan(const float* a, long long lda, const int* na_rows, const float* b, long long ldb, const int* nb_rows,
                  int B, int Ta, int Tb, const double* factors, int F, int L, int min_overlap, double* r, int* n,
                  void* stream);

/* ---- nearest-neighbour queries between two sets of rows (metrics.py; no counterpart in the
 * reference) -------------------------------------------------------------------------------------------------------
 * Rows are fp32 vectors of dimension D in [1, 128], ld* floats apart (a column block of a wider buffer is taken in
 * place). d2(x, y) = sum_d (x_d - y_d)^2: the difference in fp32, one fmaf chain over d ascending from 0, never the Gram
 * identity. d2(x, y) and d2(y, x) are the same bits; a row's results depend on no other query row of the call, nor on how
 * the library tiles or splits the work; no atomics: results are bit-identical from run to run. All comparisons are on
 * squared distances. Non-finite inputs neither hang nor fault; what they give is unspecified. A null or a host pointer
 * is refused (M2D_ERR_ARG, nothing launched).
 *
 * m2d_knn_radii: r2[i] = the k-th smallest of d2(X_i, X_j) over j != i - the row itself is excluded by INDEX, duplicates
 * of it count, with their multiplicity. M2D_ERR_ARG: k outside [1, m2d_knn_max_k()] (10), N <= k, D outside [1, 128],
 * ldx < D; M2D_ERR_WORKSPACE: ws too small.
 *
 * m2d_ball_query, per query row j of Q (M rows) against P (N rows):
 *   count[j]  = #{i : d2(Q_j, P_i) <= r2[i]}  (inclusive; r2 (N) and count (M) are given together or both NULL),
 *   nn_d2[j]  = min_i d2(Q_j, P_i),  nn_idx[j] = the smallest i that attains it.
 * M2D_ERR_ARG: M or N <= 0, D outside [1, 128], a stride below D, only one of r2 / count; M2D_ERR_WORKSPACE.
 * Both: two launches on `stream` (the tiles, each workgroup over its share of the reference rows, into the workspace;
 * then the merge in ascending order of the shares), no host synchronisation. */
int m2d_knn_max_k(void);
size_t m2d_knn_radii_workspace_bytes(int N, int k);
int m2d_knn_radii(const float* X, long long ldx, int N, int D, int k, float* r2, void* ws, size_t ws_bytes, void* stream);
size_t m2d_ball_query_workspace_bytes(int M, int N);
int m2d_ball_query(const float* Q, long long ldq, int M, const float* P, long long ldp, int N, int D, const float* r2,
                   int* count, float* nn_d2, int* nn_idx, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* M2D_H */
