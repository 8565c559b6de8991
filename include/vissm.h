/*
 * vissm.h -- C ABI of libvissm.so, the MI355X (gfx950) kernels of the
 * neural-moving-average variational-inference ELBO step.
 *
 * The reference (mehrnazmo/VIforSSMs) is TensorFlow-1.8 Python: it has no FFI.
 * Every entry point below replaces a group of TF ops that the reference builds
 * inside VI_SSM.build_flow() and runs each step through sess.run (AR.py:300-301);
 * the reference interface each one replaces is cited next to it.  The Python
 * host (viforssms_amd/, loaded through ctypes) mirrors the reference's
 * Python API on top of these calls: VI_SSM / Flow_Stack / IAF (AR.py:24-362,
 * lotka_volterra_partial.py, SV_dense.py, fitz_nag_NVP.py) and
 * optimisers.adamax.AdamaxOptimizer (optimisers/adamax.py:11-61).
 *
 * Conventions
 *   - every buffer is a caller-owned DEVICE pointer (fp32 unless stated);
 *     layouts are row-major with the TF variable layouts for weights
 *     (dense [in][out], conv1d [k][C_in][C_out]).
 *   - every call takes the HIP stream to launch on (hipStream_t passed as
 *     void*); there is no implicit device synchronisation, no hipSetDevice and
 *     no allocation on the call path: scratch comes from a caller workspace
 *     sized by the matching *_workspace_size() query.
 *   - return value 0 = OK, negative = error (VISSM_E*); vissm_last_error()
 *     returns a thread-local message for the last failing call.  Nothing
 *     throws across the ABI and nothing exits.
 *   - reductions are fixed-order (partial slabs + ordered tree), so results
 *     are bitwise reproducible run to run; no float atomics.
 */
#ifndef VISSM_H
#define VISSM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VISSM_OK 0
#define VISSM_EINVAL (-1)   /* bad shape / argument */
#define VISSM_ELAUNCH (-2)  /* HIP launch or runtime failure */
#define VISSM_EWORKSPACE (-3)

#define VISSM_PREC_FP32 0     /* exact fp32 arithmetic */
#define VISSM_PREC_BF16 1     /* bf16 MFMA operands, fp32 accumulation */
#define VISSM_PREC_BF16X3 2   /* split-bf16 (hi/lo) MFMA operands: ~fp32 products */
#define VISSM_PREC_BF16X2 3   /* split-bf16 weights, bf16 activations: every product with a weight operand as
                                 w_hi x + w_lo x (two MFMAs), the forward, the backward's recompute and its chain
                                 (W dZ, w_eps dA0, the head backward) alike; the weight-gradient products
                                 (activation x gradient) single bf16.  ELBO within 1e-4 and gradient within 1e-3 of
                                 the float64 oracle at the AR configurations (one hidden layer, k <= 32) */
#define VISSM_PREC_BF16X2_BF16 4  /* vissm_flow_ar_elbo_fused only: the recompute (x, log sigma) on split weights,
                                     the backward products bf16 -- the last flow of a step whose forward runs at
                                     VISSM_PREC_BF16X2 and backward at VISSM_PREC_BF16 (k <= 8, one window) */

const char* vissm_last_error(void);
int vissm_version(void);
/* sha256 (hex) of the sources the library was built from (viforssms_amd/srchash.py); the Python host refuses a
 * library whose hash differs from its source tree.  vissm_build_flags: extra compile flags of an A/B build ("" for
 * the production build). */
const char* vissm_source_hash(void);
const char* vissm_build_flags(void);

/* ---------------------------------------------------------------------------
 * Base noise: init_dist.slp (AR.py:24-35; lotka_volterra_partial.py:25-36).
 * eps[b][j] ~ N(0,1) from counter-based Philox4x32-10 keyed by (seed, offset+b),
 * base_lp[b] = sum_{j >= L - n_last} log N(eps[b][j]; 0, 1).
 *
 * The stream, bit for bit (tests/philox_ref.py restates it from the paper; the integer part is
 * csrc/rng_math.hpp): with r = offset + b (64-bit, wrapping) and g = j / 4,
 *   (x, y, z, w) = philox4x32_10(ctr = (g, 0, lo32(r), hi32(r)), key = (lo32(seed), hi32(seed))),
 *   u_v = ((v >> 8) + 1) * 2^-24 for each word v, so u in (0, 1], exact in fp32,
 *   columns 4g .. 4g+3 = (r1 cos 2 pi u_y, r1 sin 2 pi u_y, r2 cos 2 pi u_w, r2 sin 2 pi u_w),
 *   r1 = sqrt(-2 ln u_x), r2 = sqrt(-2 ln u_z);
 * a last group cut by L keeps its first L - 4g columns.  The stream does not depend on B, L, the launch
 * geometry or how rows are sharded over ranks.
 * ------------------------------------------------------------------------- */
int vissm_normal_base(uint64_t seed, uint64_t offset, float* eps, float* base_lp,
                      int32_t B, int32_t L, int32_t n_last, void* stream);

/* As vissm_normal_base with the row offset read from device memory (*offset_dev): a captured
 * HIP graph of the training step advances it on the device between replays. */
int vissm_normal_base_dev(uint64_t seed, const uint64_t* offset_dev, float* eps, float* base_lp,
                          int32_t B, int32_t L, int32_t n_last, void* stream);

/* base_lp only, for caller-supplied eps (parity mode). */
int vissm_base_logprob(const float* eps, float* base_lp, int32_t B, int32_t L,
                       int32_t n_last, void* stream);

/* ---------------------------------------------------------------------------
 * One IAF flow of the neural-MA sampler: IAF._create_flow + IAF.slp
 * (AR.py:50-89; lotka_volterra_partial.py:68-108 stride-2/BN variant;
 *  SV_dense.py:50-89; fitz_nag_NVP.py:68-109) with the window-shared part of
 * the first conv (feature branch, conv over features, conv bias) and the theta
 * branch precomputed by the caller:
 *
 *   a0[b,m,:] = C[win[b], m, :] + theta_term[b, :] + sum_j u[b, s*m + j] * w_eps[j, :]
 *   x_0 = elu(a0);  x_{l+1} = bn_l(elu(x_l W_l + b_l))     (l < n_hidden)
 *   (mu, r) = x_nh W_head + b_head;  sigma = softplus(r) + 1e-10
 *   stride 1: u_next[t] = u[t+k] * sigma[t] + mu[t]
 *   stride 2: u_next[2m] = u[2m+k];  u_next[2m+1] = u[2m+1+k] * sigma[m] + mu[m]
 *   logsig[b] = sum of log sigma over the last n_logsig outputs.
 * swap_out != 0 writes u_next with adjacent pairs swapped (the Permute flow of
 * the 2-D models, lotka_volterra_partial.py:137-159, fused into the store).
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t B;          /* samples (reference p) */
  int32_t L;          /* input length per sample; output length is L - k */
  int32_t k;          /* kernel_len, 1..64 */
  int32_t H;          /* network_dims[i], 1..64 (all equal) */
  int32_t n_hidden;   /* len(network_dims) - 2, 0..4 */
  int32_t bn;         /* batch_normalization(training=False) after each hidden ELU */
  int32_t stride2;    /* 2-D interleaved head (stride 2, (0,1) interleave) */
  int32_t swap_out;   /* fuse the pair-swap permutation into the output store */
  int32_t n_logsig;   /* trailing outputs counted in log q: M (1-D) or 2M (2-D) */
  int32_t n_win;      /* windows in C (1 when every sample shares one window) */
  int32_t precision;  /* VISSM_PREC_* */
  int32_t chunk_tiles; /* 0 = automatic launch geometry; > 0 = head-position tiles per t-chunk of
                          a work item (the kernel's tile size; raised to the halo minimum).  Lets a
                          small batch run the chunk geometry of a large one: a parity test at B = 20
                          walks the ~160-tile chunks the B = 65536 benchmark launch walks. */
  int32_t u_pitch;    /* row stride of u and du in floats (0 = L; else >= L).  A caller that pads rows to
                         16 floats (64 bytes) gets aligned du stores from the t-chunks of the two-sample
                         bf16 backward, which otherwise straddle 32-byte write sectors (+55 % du bytes). */
  int32_t out_pitch;  /* row stride of u_next / du_next in floats (0 = L - k; else >= L - k); the fused
                         AR(1) last flow writes x dense [B][M+1] and takes 0 or L - k */
} VissmFlowDesc;

typedef struct {
  const float* w_eps;   /* [k][H]      conv1d kernel, input channel 0 (the sample) */
  const float* w_hid;   /* [n_hidden][H][H] conv1d k=1 kernels */
  const float* b_hid;   /* [n_hidden][H] */
  const float* bn_g;    /* [n_hidden][H] or NULL (bn == 0) */
  const float* bn_b;    /* [n_hidden][H] or NULL */
  const float* w_head;  /* [H][2]  (col 0 = mu, col 1 = sigma pre-softplus) */
  const float* b_head;  /* [2] */
  /* Optional factorization of the theta branch (AR.py:63-68: three linear dense layers, so
   * theta_term = theta_x w_theta + b_theta exactly).  theta_rank = 0 (or NULL pointers): unused.
   * With 1 <= theta_rank <= 5 the bf16 AR kernels (one hidden layer, k <= 16, one window) form the
   * theta term inside their layer-0 matrix product (split-bf16 theta and w_theta in its unused K
   * rows) and add b_theta to C, instead of reading a [H] theta_term row per sample and unit; every
   * other kernel reads theta_term.  theta_term must still be passed and equal the product. */
  const float* theta_x; /* [B][theta_rank] per-sample theta (the q(theta) draw) */
  const float* w_theta; /* [theta_rank][H] collapsed weight W0 W1 W2 */
  const float* b_theta; /* [H] collapsed bias */
  int32_t theta_rank;
} VissmFlowParams;

typedef struct {        /* outputs of the backward: written, not accumulated */
  float* w_eps; float* w_hid; float* b_hid; float* bn_g; float* bn_b;
  float* w_head; float* b_head;
} VissmFlowGrads;

/* C is [n_win][Lh][H] with Lh = (L-k) (stride 1) or (L-k)/2 (stride 2);
 * win is [B] int32 window index per sample (NULL = all 0). */
size_t vissm_flow_workspace_size(const VissmFlowDesc* d, int32_t backward);

/* The launch geometry the flow kernels pick for d (host-side arithmetic, no GPU call): out[0] = head
 * positions per tile, out[1] = tiles per t-chunk of a work item, out[2] = t-chunks, out[3] = sample
 * groups.  which: 0 vissm_flow_fwd, 1 vissm_flow_bwd, 2 vissm_flow_ar_elbo_fused.  No reference
 * equivalent (TF1 has no launch geometry): the parity tests read it at a benchmark batch and pass
 * out[1] as chunk_tiles at a small one. */
int vissm_flow_geometry(const VissmFlowDesc* d, int32_t which, int32_t* out);

/* The precision vissm_flow_fwd / vissm_flow_bwd compute a descriptor in: its own where the matrix-core kernels cover
 * the shape, VISSM_PREC_FP32 where the call falls back to the exact-fp32 kernels (bf16 / bf16x3 / bf16x2 requests
 * beyond flow5's shapes: never less precise than asked; du must then be non-NULL).  Host arithmetic, no GPU;
 * VISSM_EINVAL for an invalid descriptor or VISSM_PREC_BF16X2_BF16 (a fused-flow precision). */
int32_t vissm_flow_kernel_precision(const VissmFlowDesc* d);

int vissm_flow_fwd(const VissmFlowDesc* d, const VissmFlowParams* w,
                   const float* u, const float* C, const int32_t* win,
                   const float* theta_term, float* u_next, float* logsig,
                   void* workspace, size_t ws_bytes, void* stream);

/* Backward of vissm_flow_fwd for a scalar loss.  du_next = dLoss/du_next (in
 * the stored, possibly swapped layout), dlogsig[b] = dLoss/dlogsig[b].
 * Writes du [B][L], dC [n_win][Lh][H], dtheta_term [B][H] and the weight
 * gradients.  du may be NULL on the bf16 / bf16x3 kernels when the gradient
 * w.r.t. u is not wanted (the first flow: u is the base noise). */
int vissm_flow_bwd(const VissmFlowDesc* d, const VissmFlowParams* w,
                   const float* u, const float* C, const int32_t* win,
                   const float* theta_term, const float* du_next,
                   const float* dlogsig, float* du, float* dC,
                   float* dtheta_term, const VissmFlowGrads* g,
                   void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * The last flow of the AR(1) stack fused with its ELBO terms: forward AND backward of
 * IAF._create_flow / IAF.slp (AR.py:50-89) for the final flow together with VI_SSM._ELBO's
 * AR(1) transition and observation terms (AR.py:168-176), for the loss
 *     loss = -scale * sum_b (sde_b + obs_b + logsig_b)        (scale = T / M, AR.py:184)
 * i.e. the part of -sum_b ELBO_b (AR.py:228-229) that depends on this flow.  The kernel
 * recomputes the flow's output x = u_next itself and evaluates the gradient of the AR(1) terms
 * on the fly, so vissm_flow_fwd for this flow and the ELBO backward's dz are not needed.  theta is
 * the per-sample AR(1) theta [B][3], obs / obs_bin the per-window feeds [n_win][M] (M = L - k - 1).
 * Writes x [B][M+1] (the latent path; the caller takes sde / obs and their theta gradient from it
 * with vissm_elbo_fwd / vissm_elbo_bwd), logsig [B] (the n_logsig counted outputs), du [B][L],
 * dC [n_win][Lh][H], dtheta_term [B][H] and the weight gradients of the loss.
 * Supported: bf16 / bf16x3, one hidden layer, no BN, stride 1, k <= 32. */
int32_t vissm_flow_ar_elbo_fused_supported(const VissmFlowDesc* d);
size_t vissm_flow_ar_elbo_fused_workspace_size(const VissmFlowDesc* d);
int vissm_flow_ar_elbo_fused(const VissmFlowDesc* d, const VissmFlowParams* w,
                             const float* u, const float* C, const int32_t* win,
                             const float* theta_term, const float* theta,
                             const float* obs, const float* obs_bin, float obs_std,
                             float scale, float* x, float* logsig, float* du,
                             float* dC, float* dtheta_term, const VissmFlowGrads* g,
                             void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * ELBO log-densities over a path, one model per id:
 *   AR  : VI_SSM._ELBO obs + AR(1) terms (AR.py:168-176)
 *   LV  : softplus transform + ILDJ (lotka_volterra_partial.py:290-297),
 *         obs N(.,1) and Cholesky EM density (lotka_volterra_partial.py:234-261)
 *   SV  : dim-one concat + mask/shift (SV_dense.py:245-246), diag EM density (SV_dense.py:203-223)
 *   FHN : obs N(.,0.1) and diag EM density (fitz_nag_NVP.py:232-255)
 * z is the flow output [B][D*(M+1)] (2-D models interleaved t-major).
 * Outputs per sample: sde[b], obs[b] (0 for SV) and extra[b] (LV: ILDJ, else 0).
 * ------------------------------------------------------------------------- */
#define VISSM_MODEL_AR 0
#define VISSM_MODEL_LV 1
#define VISSM_MODEL_SV 2
#define VISSM_MODEL_FHN 3
/* state coordinates S and theta length P of a model id */
#define VISSM_MODEL_S(model) ((model) == VISSM_MODEL_AR ? 1 : 2)
#define VISSM_MODEL_P(model) ((model) == VISSM_MODEL_SV ? 4 : (model) == VISSM_MODEL_FHN ? 5 : 3)

typedef struct {
  int32_t model;
  int32_t B;
  int32_t M;          /* transitions per path (reference batch_dims) */
  int32_t n_win;
  float dt;           /* Euler-Maruyama step (LV/SV/FHN) */
  float obs_std;      /* AR observation sd */
} VissmElboDesc;

typedef struct {
  const int32_t* win;     /* [B] or NULL */
  const float* obs;       /* [n_win][D][M] observation window (AR: [n_win][M]) */
  const float* obs_bin;   /* [n_win][D][M] observation mask */
  const float* mask;      /* LV [n_win][2][M+1]; SV [n_win][M+1]; else NULL */
  const float* shift;     /* same shape as mask */
  const float* dim_one;   /* SV observed coordinate [n_win][M+1]; else NULL */
  const int32_t* plain_from; /* LV / SV, optional [n_win]: from this element on, the window's mask is 1 and its
                                shift 0 (the state is softplus(z) / z itself: the reference's windows pin x_0 only,
                                lotka_volterra_partial.py:381-384, SV_dense.py:322-328); NULL: mask / shift read
                                everywhere.  vissm_elbo_fwd_grad skips their loads and the general transform there. */
  const int32_t* obs_list;   /* LV / FHN, optional [n_win][obs_stride]: the elements e in [1, M] whose observation row
                                e - 1 has a nonzero obs_bin in either coordinate, ascending, padded with -1 (the
                                reference's obs_bin files are sparse: dat/LV_obs_binary.txt, loaded at
                                lotka_volterra_partial.py:481-487, observes every 100th step; fitz_nag_NVP.py:468-473
                                loads its own); NULL: the obs rows are read at every element.  With it
                                vissm_elbo_fwd_grad evaluates the observation term at the listed elements only. */
  int32_t obs_stride;        /* entries per window in obs_list */
} VissmElboData;

int vissm_elbo_fwd(const VissmElboDesc* d, const VissmElboData* data,
                   const float* z, const float* theta, float* sde, float* obs,
                   float* extra, void* stream);

/* dLoss/d(sde, obs, extra) per sample -> dz [B][D*(M+1)], dtheta [B][P_theta].  dz may be NULL
 * (only dtheta wanted, e.g. after vissm_flow_ar_elbo_fused, which differentiates through x itself). */
int vissm_elbo_bwd(const VissmElboDesc* d, const VissmElboData* data,
                   const float* z, const float* theta, const float* g_sde,
                   const float* g_obs, const float* g_extra, float* dz,
                   float* dtheta, void* stream);

/* vissm_elbo_fwd and the theta gradient of vissm_elbo_bwd with dz = NULL, for a path z that is a
 * constant (the training step after vissm_flow_ar_elbo_fused): sde, obs (and extra) per sample and
 * dtheta = d(g_sde . sde + g_obs . obs + g_extra . extra)/dtheta.  AR(1): one pass over z (the two calls
 * would read it twice); other models: the two calls.  Same reference terms as vissm_elbo_fwd. */
int vissm_elbo_fwd_theta_grad(const VissmElboDesc* d, const VissmElboData* data, const float* z,
                              const float* theta, const float* g_sde, const float* g_obs,
                              const float* g_extra, float* sde, float* obs, float* extra,
                              float* dtheta, void* stream);

/* vissm_elbo_fwd and vissm_elbo_bwd in ONE pass over z, for upstream gradients known before the forward (the
 * training step's loss -sum_b ELBO_b: g_sde = -scale, g_obs = -scale, g_extra = +scale per sample): sde, obs,
 * extra (obs / extra may be NULL), dz and dtheta, every element's transition, obs row and ILDJ term evaluated once
 * (the forward values are the backward's own transition records).  Replaces the two launches of the ELBO
 * (AR.py:168-187, lotka_volterra_partial.py:234-297, SV_dense.py:203-232, fitz_nag_NVP.py:232-265 and their
 * tf.gradients) for every model. */
int vissm_elbo_fwd_grad(const VissmElboDesc* d, const VissmElboData* data, const float* z, const float* theta,
                        const float* g_sde, const float* g_obs, const float* g_extra, float* sde, float* obs,
                        float* extra, float* dz, float* dtheta, void* stream);

/* vissm_elbo_fwd_grad with the LV / SV / FHN kernel's waves per trajectory given by the caller instead of the
 * library's choice (its per-model default, or VISSM_ELBO_NWV): nwv waves of a block share one trajectory, each taking
 * a contiguous range of the chunk loop.  vissm_elbo_fwd_grad is this call at the library's choice.  Refused before
 * any launch: nwv not 1, 2 or 4; nwv > 1 for AR (its kernel has one wave per trajectory); nwv > 1 together with
 * data->obs_list on LV / FHN (the list's post-pass needs the whole row in one wave). */
int vissm_elbo_fwd_grad_nwv(const VissmElboDesc* d, const VissmElboData* data, const float* z, const float* theta,
                            const float* g_sde, const float* g_obs, const float* g_extra, float* sde, float* obs,
                            float* extra, float* dz, float* dtheta, int32_t nwv, void* stream);

/* ---------------------------------------------------------------------------
 * Global-norm clip + Adamax over one flat parameter buffer:
 * tf.global_norm / tf.clip_by_global_norm (AR.py:230-232) followed by
 * AdamaxOptimizer._apply_dense (optimisers/adamax.py:42-58):
 *   g <- g * clip * min(1/||g||, 1/clip)   (NaN when ||g|| is not finite)
 *   v <- beta1 v + (1-beta1) g ;  m <- max(beta2 m + eps, |g|) ;  p <- p - lr v/m
 * clip <= 0 disables clipping.  gnorm_out (device, 1 float, may be NULL)
 * receives ||g|| before clipping.
 * ------------------------------------------------------------------------- */
size_t vissm_adamax_workspace_size(int64_t n);
int vissm_adamax_step(float* params, const float* grads, float* v, float* m,
                      int64_t n, float lr, float beta1, float beta2, float eps,
                      float clip, float* gnorm_out, void* workspace,
                      size_t ws_bytes, void* stream);

/* As vissm_adamax_step, with the non-finite guard of the training loop: when ||g||
 * is not finite -- where tf.clip_by_global_norm would write NaN into every variable
 * (AR.py:230-232) -- params, v and m are left untouched and *skipped (device int32, may be NULL)
 * is incremented.  The decision is made on the device: no host synchronisation. */
int vissm_adamax_step_guarded(float* params, const float* grads, float* v, float* m,
                              int64_t n, float lr, float beta1, float beta2, float eps,
                              float clip, float* gnorm_out, int32_t* skipped, void* workspace,
                              size_t ws_bytes, void* stream);

/* Sum of squares of a flat buffer (fixed-order), result to out[0] (device float). */
int vissm_sqnorm(const float* x, int64_t n, float* out, void* workspace,
                 size_t ws_bytes, void* stream);

/* out[c] = sum_r slab[r][c] for r = 0..R-1 in fixed order (deterministic reduce). */
int vissm_reduce_rows(const float* slab, float* out, int64_t R, int64_t N,
                      void* stream);

/* The same over a bf16 slab (each element widened to fp32, rows summed in order r = 0..R-1 in
 * fp32): the flow backward's window-shared dC partials at bf16 products (one row per 16-sample
 * group: 4096 rows at the B = 65536 benchmark), exported for its parity test. */
int vissm_reduce_rows_bf16(const void* slab, float* out, int64_t R, int64_t N, void* stream);

/* x[0..n) = hi + lo (bf16 planes, hi = bf16(x), lo = bf16(x - hi), round to nearest even): the operands of the
 * split-bf16 GEMMs of LV's window-shared conv over its time-mixing features (no reference equivalent: the
 * reference runs that conv in fp32, lotka_volterra_partial.py:78-82).  x 16-byte aligned, hi / lo 8-byte. */
int vissm_split_bf16(const float* x, void* hi, void* lo, int64_t n, void* stream);

/* ---------------------------------------------------------------------------
 * Window-shared feature branch + the first conv's feature channels (AR.py:53-62;
 * SV_dense.py:53-62; fitz_nag_NVP.py:71-79): per window w,
 *   F = elu(elu(elu(elu(h0 W0 + b0) W1 + b1) W2 + b2) W3 + b3)        [Lf][H]
 *   C[w][m][o] = conv_b[o] + sum_{j<k} sum_{i<H} F[s m + j][i] conv_w[j][1 + i][o],  m < Lh
 * (the sample channel conv_w[j][0][:] is the flow kernel's w_eps).  h0: the window's
 * time-feature rows, Lf rows of Cin floats, windows in_win_stride floats apart.
 * fwd writes C [n_win][Lh][H] and the four layer outputs act [4][n_win][Lf][H] (rows
 * s (Lh - 1) + k .. Lf - 1 unused); bwd takes dC and writes (not accumulates) the
 * gradients of W0..W3, b0..b3, conv_w (its sample channel 0) and conv_b.
 * Replaces the four tf.layers.dense and the feature part of tf.layers.conv1d with
 * their gradients.  Cin <= 63, H <= 64, k <= 64, stride 1 | 2; deterministic.
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t n_win, Lf, Cin, H, k, stride, Lh;
  int64_t in_win_stride;
} VissmFeatDesc;

typedef struct {
  const float* w[4];    /* W0 [Cin][H], W1..W3 [H][H] */
  const float* b[4];    /* [H] */
  const float* conv_w;  /* [k][1 + H][H] */
  const float* conv_b;  /* [H] */
} VissmFeatParams;

typedef struct {
  float* w[4];
  float* b[4];
  float* conv_w;
  float* conv_b;
} VissmFeatGrads;

size_t vissm_feat_workspace_size(const VissmFeatDesc* d);
/* The launch geometry vissm_feat_fwd (backward = 0) / vissm_feat_bwd (backward != 0) pick for d now (host-side
 * arithmetic, no GPU call; the VISSM_FEAT_KT / VISSM_FEAT_KT_BWD overrides included): out[0] = output positions per
 * block (8, 16 or 32: the kernel instantiation), out[1] = blocks per window, out[2] = dynamic LDS bytes of the
 * launch.  VISSM_EINVAL for a descriptor the kernels refuse.  No reference equivalent (TF1 has no launch geometry):
 * the tests assert through it which variant they ran. */
int vissm_feat_geometry(const VissmFeatDesc* d, int32_t backward, int32_t* out);
int vissm_feat_fwd(const VissmFeatDesc* d, const VissmFeatParams* w, const float* h0, float* C, float* act,
                   void* stream);
int vissm_feat_bwd(const VissmFeatDesc* d, const VissmFeatParams* w, const float* h0, const float* act,
                   const float* dC, const VissmFeatGrads* g, void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Lotka-Volterra's window-shared feature branch and first conv (lotka_volterra_partial.py:71-82): per window,
 *   H3 = elu(elu(elu(h0 W0 + b0) W1 + b1) W2 + b2)              [R][H]   (R = the window's time-feature rows)
 *   D  = elu(H3 W3 + b3)                                        [R][U]   (the time-mixing dense layer, transposed
 *                                                                         by the reference so that U is the conv's
 *                                                                         time axis and R its channels)
 *   C[m][h] = conv_b[h] + sum_{j<k} sum_{r<R} D[r][s m + j] conv_w[j][1 + r][h]
 * Replaces the four tf.layers.dense, the transpose and the feature part of tf.layers.conv1d with their gradients:
 * the three small layers in fp32 (vissm_lv_mlp_*), the time-mixing layer and the conv as bf16 matrix-core GEMMs
 * (vissm_gemm_bf16) on operands packed by vissm_lv_pack, the conv's diagonal sum and its transpose by
 * vissm_lv_conv_diag[_bwd], the conv weight gradient back to [k][1 + R][H] by vissm_lv_conv_wscatter
 * (viforssms_amd/ops.py LvFeatConvFn chains them).  mlp_fwd writes act [n_layers][n_win][R][H] (fp32 layer outputs)
 * and H3b [n_win][R][64] bf16 (the last layer's output, a ones column at H for W3b's bias row, zeros; H3lo, when not
 * null, the same layout holding the bf16 residual of each element, hi + lo = the fp32 value to ~2^-16); mlp_bwd
 * takes dH3 [n_win][R][ld] (columns < H) and writes the gradients of W0.., b0.. (the conv fields of the grads struct
 * unused).
 *
 * Stochastic volatility's branch (SV_dense.py:50-62: four dense + ELU layers over the window's features with their
 * first differences, then the conv over the 50 feature channels at k = 50) runs through the same entry points:
 * n_layers = 4, sv_diff = 1 (h0 is then the window's time features [L][Cr] and row r of the MLP input is
 * [h0[r + 1][0 .. Cr), h0[r + 1][c] - h0[r][c] for c < Cr - 2], so Cin = 2 Cr - 2 and R = L - 1), the conv as a
 * split-bf16 GEMM (vissm_gemm_bf16x3) on F = H3b / H3lo and the packed conv kernel (vissm_lv_pack with ldw = 0).
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t n_win, R, Cin, H;
  int64_t in_win_stride;
  int32_t n_layers;   /* dense + ELU layers in the MLP: 0 or 3 (LV), 4 (SV) */
  int32_t sv_diff;    /* 1: SV's first-difference input assembly (above) */
} VissmLvFeatDesc;

size_t vissm_lv_mlp_workspace_size(const VissmLvFeatDesc* d);
int vissm_lv_mlp_fwd(const VissmLvFeatDesc* d, const VissmFeatParams* w, const float* h0, float* act, void* H3b,
                     void* H3lo, void* stream);
int vissm_lv_mlp_bwd(const VissmLvFeatDesc* d, const VissmFeatParams* w, const float* h0, const float* act,
                     const float* dH3, int ld_dH3, const VissmFeatGrads* g, void* workspace, size_t ws_bytes,
                     void* stream);
/* W3b [64][ldw] bf16 (rows < H: w3 [H][U], row H: b3, zeros; columns >= U zero; ldw = 0: none, w3 / b3 / W3b
 * unused) and Wc [R][ldc] bf16 (Wc[r][j H + h] = conv_w[j][1 + r][h], zero for columns >= k H); W3b_lo / Wc_lo,
 * when not null, their bf16 residual planes (the split-bf16 GEMM's operands) */
int vissm_lv_pack(const float* w3, const float* b3, int H, int U, int ldw, void* W3b, void* W3b_lo, const float* conv_w,
                  int R, int k, int ldc, void* Wc, void* Wc_lo, void* stream);
/* C[m][h] = conv_b[h] + sum_{j<k} G[s m + j][j H + h], G [U][ldg] fp32, m < Lh */
int vissm_lv_conv_diag(const float* G, int ldg, const float* conv_b, int H, int k, int stride, int Lh, float* C,
                       void* stream);
/* its transpose: dG[u][j H + h] = dC[(u - j) / s][h] where that is a position (bf16 [U][ldg], zero elsewhere; dG_lo,
 * when not null, the bf16 residual plane), and dconv_b[h] = sum_m dC[m][h] */
int vissm_lv_conv_diag_bwd(const float* dC, int H, int k, int stride, int Lh, int U, int ldg, void* dG, void* dG_lo,
                           float* dconv_b, void* stream);
/* dconv_w[j][1 + r][h] = dWc[r][j H + h]; channel 0 (the flow kernel's w_eps) = 0 */
int vissm_lv_conv_wscatter(const float* dWc, int ldc, int R, int k, int H, float* dconv_w, void* stream);

/* ---------------------------------------------------------------------------
 * bf16 matrix-core GEMM: C[m][n] = sum_k A[m][k] B[k][n], fp32 accumulation (the LV feature branch's products).
 * A: a_kmajor = 0: A[m][k] at A[m lda + k]; 1: at A[k lda + m].  B: b_kmajor = 0: B[k][n] at B[n ldb + k]; 1: at
 * B[k ldb + n].  lda, ldb multiples of 8, A and B 16-byte aligned.  Epilogues: VISSM_GEMM_F32 (fp32 C[m ldc + n]),
 * VISSM_GEMM_ELU_BF16 (bf16 elu(acc)), VISSM_GEMM_DELU_BF16 (bf16 acc * elu'(y), y = aux[m ldc + n] a bf16 ELU
 * output: y < 0 ? y + 1 : 1).  split_k > 1 (fp32 epilogue, ldc == N): per-split partials in the workspace summed in
 * split order (deterministic).
 * ------------------------------------------------------------------------- */
#define VISSM_GEMM_F32 0
#define VISSM_GEMM_ELU_BF16 1
#define VISSM_GEMM_DELU_BF16 2
typedef struct {
  int64_t M, N, K, lda, ldb, ldc;
  int32_t a_kmajor, b_kmajor, epilogue, split_k;
} VissmGemmDesc;

size_t vissm_gemm_workspace_size(const VissmGemmDesc* d);
int vissm_gemm_bf16(const VissmGemmDesc* d, const void* A, const void* B, void* C, const void* aux, void* workspace,
                    size_t ws_bytes, void* stream);
/* The split-bf16 form (fp32-class products: the operands' hi / lo bf16 planes, x = hi + lo to ~2^-16, the same
 * layouts): C = A_hi B_hi + A_hi B_lo + A_lo B_hi, one launch whose K loop runs the three passes (split-K divides
 * the 3 K range).  Every epilogue: the bf16 ones write C as a hi / lo plane pair (the lo plane at C + M ldc) and
 * read aux the same way (y = aux_hi + aux_lo). */
size_t vissm_gemm_bf16x3_workspace_size(const VissmGemmDesc* d);
int vissm_gemm_bf16x3(const VissmGemmDesc* d, const void* A_hi, const void* A_lo, const void* B_hi, const void* B_lo,
                      void* C, const void* aux, void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Window gather: the per-step feed assembly of VI_SSM.train (AR.py:267-288;
 * lotka_volterra_partial.py:366-386; SV_dense.py:304-328) from device-resident
 * padded channel tables (built once, AR.py:135-150), keyed by the step's window
 * starts (batch_select):
 *   out[r*os_r + j*os_j + c*os_c] = src[c*c_pitch + stride*starts[r] + offset + j*j_step]
 * for r < n, j < len, c < C.  time_feats [n][kernel_ext][C]: c_pitch = table
 * length, os = (kernel_ext*C, C, 1); per-window feeds [n][D][len] from a [D][..]
 * table: os = (D*len, 1, len).  The caller guarantees every source index lies in
 * the table (the reference's starts come from arange(0, T, M)).
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t n, len, C;        /* windows, positions per window, channels */
  int32_t stride;           /* start multiplier (2 for the interleaved 2-D series) */
  int64_t offset, j_step, c_pitch;
  int64_t os_r, os_j, os_c; /* output strides (elements) */
} VissmGatherDesc;

int vissm_gather_windows(const VissmGatherDesc* d, const float* src, const int32_t* starts,
                         float* out, void* stream);

/* ---------------------------------------------------------------------------
 * q(theta): the variational posterior over the SDE parameters (AR.py:376-391;
 * lotka_volterra_partial.py:494-508; SV_dense.py:428-442; fitz_nag_NVP.py:480-494):
 * n_bij bijectors Invert(MaskedAutoregressiveFlow(MADE [5, 5, 5], elu | relu)) with
 * Permute between them over a Normal(base_loc, base_scale) base of P dimensions.
 *   fwd: theta [B][P] = chain(x0), logq [B] = log q(theta) (base log-prob + sum of
 *        the clipped log-scales, clip [-5, 3] straight-through).
 *   bwd: dw += d loss / d w for d loss / d theta = dtheta and d loss / d logq = dlogq
 *        (either may be NULL = 0); deterministic (fixed-order sums).
 * w, mask: every bijector's MADE variables in the parameter store's order -- dense0
 * kernel [P][5], bias [5], dense1 [5][5], bias, dense2 [5][5], bias, dense3 [5][2P],
 * bias [2P] -- vissm_theta_num_params(P, n_bij) floats; mask holds the MADE masks in
 * the same layout (1 on the biases).  perm[i][q]: after bijector i, z[q] <- z[perm[i][q]].
 * ------------------------------------------------------------------------- */
#define VISSM_THETA_MAX_P 5
#define VISSM_THETA_MAX_BIJ 8
typedef struct {
  int32_t B, P, n_bij, relu;  /* relu: 0 = elu (AR / LV / FHN), 1 = relu (SV) */
  float base_loc, base_scale;
  int32_t perm[VISSM_THETA_MAX_BIJ - 1][VISSM_THETA_MAX_P];
} VissmThetaDesc;

int32_t vissm_theta_num_params(int32_t P, int32_t n_bij);
size_t vissm_theta_workspace_size(const VissmThetaDesc* d);
int vissm_theta_fwd(const VissmThetaDesc* d, const float* w, const float* mask, const float* x0,
                    float* theta, float* logq, void* stream);
int vissm_theta_bwd(const VissmThetaDesc* d, const float* w, const float* mask, const float* x0,
                    const float* dtheta, const float* dlogq, float* dw, void* workspace,
                    size_t ws_bytes, void* stream);

/* The flows' theta branch backward (IAF._create_flow's three linear dense layers on theta, AR.py:63-68;
 * lotka_volterra_partial.py:84-89): theta_term = ((theta W0 + b0) W1 + b1) W2 + b2 with W0 [P][n0], W1 [n0][n1],
 * W2 [n1][H]; given dterm = d loss / d theta_term [B][H] it writes dtheta [B][P] and the six weight gradients
 * (overwritten, not accumulated).  P <= 8, n0 / n1 / H <= 64; deterministic (fixed-order sums); workspace from
 * vissm_theta_branch_bwd_workspace_size(B, P) (0: bad shape). */
/* its forward: the collapsed weights Wc = W0 W1 W2 [P][H], bc = (b0 W1 + b1) W2 + b2 [H] (the factors the AR flow
 * kernels fold into their layer-0 product, VissmFlowParams.theta_rank) and, when theta_term is not NULL,
 * theta_term = theta Wc + bc [B][H]. */
int vissm_theta_branch_fwd(int32_t B, int32_t P, int32_t n0, int32_t n1, int32_t H, const float* theta,
                           const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                           const float* b2, float* Wc, float* bc, float* theta_term, void* stream);
size_t vissm_theta_branch_bwd_workspace_size(int32_t B, int32_t P);
int vissm_theta_branch_bwd(int32_t B, int32_t P, int32_t n0, int32_t n1, int32_t H, const float* theta,
                           const float* dterm, const float* W0, const float* b0, const float* W1, const float* b1,
                           const float* W2, float* dtheta, float* dW0, float* db0, float* dW1, float* db1,
                           float* dW2, float* db2, void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Column statistics of a sample-major matrix: posterior summaries computed where
 * the samples are.  They replace the reference's host path from posterior samples
 * to credible bands -- VI_SSM.save_paths writes every sample of every window with
 * np.savetxt (AR.py:323-362) and vis.py takes the quantiles of that file offline.
 *
 * x is [B][pitch] fp32, columns 0..n_cols-1 used, pitch >= n_cols; the base pointer
 * needs only the 4-byte alignment of its elements (x[:, 1:]-style views).
 *
 * Moments: sums[0][c] = sum of x[b][c], sums[1][c] = sum of squares, both over the
 * non-NaN entries in double, n_valid[c] their count.  Per-row-slab partials in the
 * workspace, then a fixed-order sum: bitwise reproducible, no float atomics.
 *
 * Order statistics: an exact 4-pass byte-wise radix select on the order key
 *   -0 -> +0; any NaN -> 0xFFFFFFFF; else, with b the float's bits,
 *   key = (b >> 31) ? ~b : (b | 0x80000000)
 * whose unsigned order is numpy's sort order (-inf .. +inf, NaN last).  Each column
 * has n_ranks targets (1..16), target r asking for the element of 0-based rank
 * rank_left[c][r] of the sorted column.  Pass p = 0..3 looks at key byte 3 - p:
 *   hist:   hist[c][r][256] = counts of that byte over the elements of column c
 *           whose key bytes above it equal those of prefix[c][r] (pass 0: every
 *           element; prefix is read but its value ignored).  Overwrites hist.
 *           Integer counts: independent of the order of the adds, so the ranks of
 *           a data-parallel run SUM-all-reduce hist here and select over the
 *           union of their samples exactly, without gathering them.
 *   narrow: per (c, r) the digit d with cum[d-1] <= rank_left < cum[d] of the
 *           histogram it is given; rank_left -= cum[d-1]; prefix |= d << shift
 *           (pass 0 starts from prefix 0).  A rank outside [0, total count) is
 *           clamped to the nearest valid one.
 *   decode: out[r][c] = the float of key prefix[c][r] (0xFFFFFFFF: a quiet NaN).
 * The global sample count (all ranks' B) must stay below 2^31.  Workspace sizes:
 * host arithmetic only, 0 = bad descriptor; they depend on the number of row slabs
 * (at most 256), not on B * n_cols.
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t B, n_cols, pitch; /* rows, used columns, row pitch (elements) */
  int32_t n_ranks;          /* order-statistic targets per column, 1..16 (the moments ignore it beyond the range) */
} VissmColStatDesc;

/* replaces: the mean / sd of the host np.savetxt -> offline summary path (AR.py:323-362, vis.py) */
size_t vissm_col_moments_workspace_size(const VissmColStatDesc* d);
int vissm_col_moments(const VissmColStatDesc* d, const float* x, double* sums /* [2][n_cols] */,
                      int32_t* n_valid /* [n_cols] */, void* workspace, void* stream);
/* the four below replace: the host np.savetxt -> offline quantile path (AR.py:323-362, vis.py) */
/* scratch of the select (AR.py:323-362 / vis.py keep every sample on the host instead) */
size_t vissm_col_select_workspace_size(const VissmColStatDesc* d);
/* one byte's histograms: the counting half of vis.py's column-wise quantile over the save_paths file */
int vissm_col_select_hist(const VissmColStatDesc* d, const float* x, const uint32_t* prefix /* [n_cols][n_ranks] */,
                          int32_t pass, int32_t* hist /* [n_cols][n_ranks][256] */, void* workspace, void* stream);
/* the digit that holds each rank: the selecting half of the same quantile (AR.py:323-362, vis.py) */
int vissm_col_select_narrow(const VissmColStatDesc* d, const int32_t* hist, int32_t* rank_left /* in/out */,
                            uint32_t* prefix /* in/out */, int32_t pass, void* stream);
/* keys back to floats: the order statistics vis.py reads off the sorted file (AR.py:323-362) */
int vissm_col_select_decode(const VissmColStatDesc* d, const uint32_t* prefix, float* out /* [n_ranks][n_cols] */,
                            void* stream);

/* ---------------------------------------------------------------------------
 * Forward simulation of the four SDEs by Euler-Maruyama, one sample per lane: posterior-predictive forecasts
 * from the fitted model's per-sample theta and last latent state.  The reference has no forecast; its only forward
 * simulations are the host data generators (AR_dat_gen.py:6-43 and the one-path numpy loops that restate the
 * transition models of lotka_volterra_partial.py:244-261, SV_dense.py:203-223, fitz_nag_NVP.py:243-255), one path in
 * float64.  The step is the transition vissm_elbo_fwd scores (csrc/sim_math.hpp, theta raw: logs where the density
 * exponentiates them):
 *   AR  : x' = th1 x + th0 + e^th2 n0
 *   LV  : x' = x + dt (e0 x1 - Bv, Bv - e2 x2) + sqrt(dt) chol([[A, -Bv], [-Bv, Cc]]) n,
 *         e_i = e^th_i, Bv = e1 x1 x2, A = e0 x1 + Bv, Cc = Bv + e2 x2
 *   SV  : x1' = x1 + dt th0 x1 + sqrt(dt) x1 e^{x2/2} n0;  x2' = x2 + dt (th1 - e^th2 x2) + sqrt(dt) e^th3 n1
 *   FHN : x' = x + dt (e^th0 (x1 - x1^3 - x2 + th1), th2 x1 - x2 + 1.4) + sqrt(dt) (sqrt(e^th3) n0, sqrt(e^th4) n1)
 * with S = VISSM_MODEL_S(model) state coordinates and P = VISSM_MODEL_P(model) parameters.  A sample whose new
 * state is not finite -- for LV also one with a coordinate <= 0 -- is dead: that step and every later one of its
 * row are NaN in x, y and x_end (the column statistics leave NaN out and count n_valid).  A start state that fails
 * the same test gives a NaN row.
 *
 * Randomness: drawn in the kernel, the stream of vissm_normal_base.  Sample b at absolute step t0 + t uses entries
 * j = (t0 + t) n_stream + i of Philox row row0 + b under key seed (counter (j / 4, 0, row)), i < S the state
 * normals, then with observations S more: y[b][d][t] = x[b][d][t] + obs_std n_{S + d}.  n_stream = S without
 * observations, 2 S with them (not SV, whose first coordinate is the observed series).  So
 * vissm_normal_base(seed, row0, .., B, n_stream H_total, ..) returns the numbers consumed, whatever the launch
 * geometry, the sharding of B over ranks or the cut of the horizon into calls: t0 > 0 with x_start = the previous
 * call's x_end continues a simulation bitwise ((t0 + H) n_stream must stay below 2^31).
 *
 * x, y: [B][S][H] sample-major (what vissm_col_* summarise); x_end [B][S] the state after the last step (x_start
 * for H = 0).  Each wave stages VISSM_SIM_TILE steps of its 64 samples in LDS and writes them out row by row,
 * 64 lanes on consecutive steps of one sample.  No workspace, no atomics: bitwise reproducible.
 * ------------------------------------------------------------------------- */
#define VISSM_SIM_TILE 64
typedef struct {
  int32_t model, B, H, t0, n_stream;
  float dt, obs_std;
  int32_t with_obs;
} VissmSimDesc;

int vissm_sde_simulate(const VissmSimDesc* d, uint64_t seed, uint64_t row0,
                       const float* theta /* [B][P] */, const float* x_start /* [B][S] */,
                       float* x /* [B][S][H] */, float* y /* [B][S][H] or NULL */,
                       float* x_end /* [B][S] */, void* stream);

/* ---------------------------------------------------------------------------
 * Bootstrap particle filter of the AR, LV and FHN state-space models: an estimate of log p(y | theta) per theta row
 * and the filtering cloud, neither of which comes out of the flows.  The reference has no filter; the loop restates
 * its transition and observation models (AR.py:168-176, lotka_volterra_partial.py:234-261, fitz_nag_NVP.py:232-255)
 * as propagate / weight / resample.  SV is refused (VISSM_EINVAL): it has no observation model, the rule of
 * with_obs in vissm_sde_simulate.
 *
 * K filters, one block and one theta row each, N particles per filter (64, 128, 256, 512 or 1024: one per lane, a
 * power of two), H steps per call from absolute step t0.  obs, obs_bin: [S][T_total] fp32, shared by all filters and
 * indexed by absolute step; observation t scores the state after transition t (row e - 1 of element e in
 * vissm_elbo_fwd's alignment).  t0 + H <= T_total and (t0 + H) S < 2^31.
 *
 * Step t0 + t: (1) the step of vissm_sde_simulate with its death rule; particle (k, i) consumes exactly the normals
 * that call gives row row0 + k N + i with n_stream = S (counter (j / 4, 0, row), key seed).  (2) If any coordinate of
 * obs_bin[:, t0 + t] is non-zero, with sums over the particles of filter k (csrc/pf_math.hpp):
 *   logw_i = sum_d bin_d log N(y_d; x_i,d, obs_std)       (coordinates with bin_d = 0 are not read)
 *   m = max over live i of logw_i;  q_i = (uint64) trunc(exp(logw_i - m) 2^40), exp in fp32; q_i = 0 for a dead
 *   particle (NaN state);  W = sum q_i, an exact integer < 2^50
 *   ll_inc = m + log W - 40 ln 2 - ln N  (double);  ess = W^2 / sum q_i^2  (double, fixed order)
 *   U = x >> 8 of philox4x32_10(ctr = (t0 + t, 1, lo32(r), hi32(r)), key = seed), r = row0 + k N
 *   tau_j = ((j 2^24 + U) W) >> (24 + log2 N);  anc[j] = #{i : C_i <= tau_j}, C the inclusive cumulative sum of q
 *   slot j takes the state of particle anc[j] and keeps its own Philox row.
 * At an unobserved step ll_inc = 0, ess = N, q_trace = 0 and anc_trace = the identity.  If W = 0 at an observed step
 * (no live particle with a non-zero weight) the filter is dead from that step on: loglik = -inf, and its cloud,
 * state_end, ll_inc and ess are NaN.  A call whose loglik_in[k] is -inf continues a dead filter.
 *
 * loglik [K] double = loglik_in (NULL: 0) + the increments; ll_inc, ess [K][H]; state_end [K N][S]; optional cloud
 * [K N][S][H], the equally weighted post-resampling particles, sample-major (what vissm_col_* summarise), staged in
 * LDS and written as row segments of 64, 32 or (LV / FHN at N = 1024) 16 consecutive steps; optional traces for
 * tests, NULL in production: q_trace [K][H][N] uint64, anc_trace [K][H][N] int32.  x_start [K N][S]: a start state
 * that fails the death rule is a dead particle.  t0 > 0 with x_start = the previous call's state_end and loglik_in =
 * its loglik continues bitwise.  No workspace, no float atomics, fixed-order double sums: two launches are bitwise
 * equal, and filter k's bits depend on (seed, row0 + k N, theta_k, N, data) only, not on K or the block index.
 * vissm_particle_filter_lds_bytes: the LDS one block declares (host arithmetic; 0 = bad model or N).
 * vissm_particle_filter_adapted, below, takes the same arguments and gives an estimate of far smaller variance where
 * obs_std is small against the process noise.
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t model, K, N, H, t0, T_total;
  float dt, obs_std;
} VissmPfDesc;

int32_t vissm_particle_filter_lds_bytes(int32_t model, int32_t N);
int vissm_particle_filter(const VissmPfDesc* d, uint64_t seed, uint64_t row0,
                          const float* theta /* [K][P] */, const float* x_start /* [K N][S] */,
                          const float* obs /* [S][T_total] */, const float* obs_bin /* [S][T_total] */,
                          const double* loglik_in /* [K] or NULL */, double* loglik /* [K] */,
                          float* ll_inc /* [K][H] */, float* ess /* [K][H] */, float* state_end /* [K N][S] */,
                          float* cloud /* [K N][S][H] or NULL */, uint64_t* q_trace /* [K][H][N] or NULL */,
                          int32_t* anc_trace /* [K][H][N] or NULL */, void* stream);

/* ---------------------------------------------------------------------------
 * Fully adapted auxiliary particle filter of the same three models: the descriptor, arguments, geometry, Philox
 * streams, integer pipeline, outputs, chaining and refusals of vissm_particle_filter, with a lower-variance estimate
 * of log p(y | theta).  The Euler-Maruyama transition is Gaussian given the previous state, x' | x ~ N(mu(x),
 * Sigma(x)), and the observation reads the coordinates O = {d : bin_d != 0} with N(0, R) noise, R = obs_std^2, so
 * both the predictive p(y_t | x_t-1) and the conditional p(x_t | x_t-1, y_t) are Gaussian (csrc/gp_math.hpp).
 *
 * An unobserved step is vissm_particle_filter's, bitwise.  At an observed step
 *   logw_i = log N(y_O; mu_O(x_i), Sigma_OO(x_i) + R I) of the particle's *pre-step* state x_i (fp32);
 *   m, q_i, W, ll_inc, ess, U, tau_j and anc[j] from these logw_i exactly as above;
 *   slot j takes the pre-step state of particle anc[j] and draws x'_j = m + L n from its conditional,
 *   m = mu + K (y_O - mu_O), K = Sigma_.O (Sigma_OO + R I)^-1, L L^T = Sigma - K Sigma_O. (lower, coordinate order),
 *   with n the S normals of its own Philox row at this step; then the death rule.
 * A coordinate is observed iff bin_d != 0 (the value is otherwise unused; the bootstrap filter multiplies by it, and
 * the two agree for 0 / 1).  The cloud holds the post-propagation particles, an equally weighted sample of
 * p(x_t | y_1:t, theta), so vissm_particle_smooth runs on it unchanged.  Unlike the bootstrap's it may hold dead (NaN)
 * particles at observed steps of LV, where a draw can leave the orthant after the resampling; they get q = 0 at the
 * next observed step, the second-stage weight of the killed model, so the estimate stays that of the model
 * vissm_particle_filter estimates.  Also refused: obs_std <= 0 or not finite (the conditional degenerates).
 * vissm_particle_filter_adapted_lds_bytes = vissm_particle_filter_lds_bytes (the same arrays).
 * ------------------------------------------------------------------------- */
int32_t vissm_particle_filter_adapted_lds_bytes(int32_t model, int32_t N);
int vissm_particle_filter_adapted(const VissmPfDesc* d, uint64_t seed, uint64_t row0,
                                  const float* theta /* [K][P] */, const float* x_start /* [K N][S] */,
                                  const float* obs /* [S][T_total] */, const float* obs_bin /* [S][T_total] */,
                                  const double* loglik_in /* [K] or NULL */, double* loglik /* [K] */,
                                  float* ll_inc /* [K][H] */, float* ess /* [K][H] */,
                                  float* state_end /* [K N][S] */, float* cloud /* [K N][S][H] or NULL */,
                                  uint64_t* q_trace /* [K][H][N] or NULL */,
                                  int32_t* anc_trace /* [K][H][N] or NULL */, void* stream);

/* ---------------------------------------------------------------------------
 * Particle smoother: forward filtering, backward simulation (FFBSi) over the cloud vissm_particle_filter wrote.  The
 * filter's bands are filtering distributions p(x_t | y_1:t, theta); the trajectories drawn here are samples of the
 * smoothing distribution p(x_1:T | y_1:T, theta), the law the variational posterior over the latent path approximates.
 * The reference has no smoother; the backward weights restate its transition models (AR.py:172-176,
 * lotka_volterra_partial.py:244-261, fitz_nag_NVP.py:243-255).  SV is refused (VISSM_EINVAL), as in the filter.
 *
 * K filters of N particles (the filter's sizes), M trajectories per filter (a power of two, 64 <= M <= N), H steps per
 * call; t0 is the absolute step of column 0 and enters the Philox counter only.  cloud [K N][S][H] holds the equally
 * weighted post-resampling particles of every step, so the backward weights are the transition densities alone.
 * Trajectory (k, j) walks t from H - 1 down; with xt its state at t + 1 (x_next[k M + j] for t = H - 1) and sums over
 * the particles i of filter k at step t (csrc/ps_math.hpp):
 *   logw_i = log p(xt | x_i, theta_k) in fp32, the value the ELBO's transition term has, less a constant of theta
 *   m = max over live i of logw_i;  q_i = (uint64) trunc(exp(logw_i - m) 2^40), exp in fp32; q_i = 0 for a dead
 *   particle (not finite; for LV a coordinate <= 0);  W = sum q_i, an exact integer <= 2^50
 *   U = x of philox4x32_10(ctr = (t0 + t, 2, lo32(r), hi32(r)), key = seed), r = row0 + k N + j, all 32 bits
 *   tau = (U W) >> 32;  idx = #{i : C_i <= tau}, C the inclusive cumulative sum of q in particle order
 *   paths[k M + j][:][t] = cloud[k N + idx][:][t], bit for bit.
 * (The normals' counters carry 0 in their second word and the filter's resampling 1: the three streams never meet.)
 * Terminal rule: with x_next = NULL, logw_i = 0 for every live particle at t = H - 1, a uniform draw over the live
 * ones.  If W = 0 -- no live particle, or a NaN target -- the trajectory is the canonical quiet NaN at that step and
 * idx = -1; a NaN target gives W = 0 at the step before it, so NaN propagates backward, and a filter that died at any
 * step (its cloud is NaN from there on) has all-NaN trajectories.
 *
 * paths [K M][S][H] sample-major (what vissm_col_* summarise); x_first [K M][S] = paths at step 0, the x_next of the
 * call over the H' steps before (its t0 smaller by H'): chained calls equal one call bitwise.  Optional idx [K M][H]
 * and, for tests, q_trace [K][H][M][N] uint64.  A block owns 64 trajectories of one filter, one per lane, grid
 * (M / 64, K); its min(4, N / 64) waves share out the particles.  The cloud is staged in LDS in tiles of 32, 16, 8 or 4
 * steps and read as row segments of that many consecutive steps, the outputs leave the same way.  No workspace, no
 * atomics; the maximum is exact in any order, the sums are integers and the selection is defined in particle order:
 * two launches are bitwise equal, and trajectory (k, j) depends on (seed, row0 + k N + j, theta_k, filter k's cloud,
 * x_next[k M + j]) only, not on K or the launch geometry.  K <= 65535, H >= 1, t0 + H < 2^31.
 * vissm_particle_smooth_lds_bytes: the LDS one block declares (host arithmetic; 0 = bad model, N or M).
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t model, K, N, M, H, t0;
  float dt;
} VissmPsDesc;

int32_t vissm_particle_smooth_lds_bytes(int32_t model, int32_t N, int32_t M);
int vissm_particle_smooth(const VissmPsDesc* d, uint64_t seed, uint64_t row0,
                          const float* theta /* [K][P] */, const float* cloud /* [K N][S][H], the filter's layout */,
                          const float* x_next /* [K M][S] or NULL: the target of step H - 1 */,
                          float* paths /* [K M][S][H] sample-major */,
                          float* x_first /* [K M][S]: paths at step 0, the next (earlier) call's x_next */,
                          int32_t* idx /* [K M][H] or NULL: the chosen particle, -1 where NaN */,
                          uint64_t* q_trace /* [K][H][M][N] or NULL: tests only */, void* stream);

/* ---------------------------------------------------------------------------
 * Particle filter and smoother of the stochastic-volatility model.  The entries above refuse SV because it has no
 * obs_std / obs_bin observation model; it can be filtered all the same: the observed series y is the first coordinate
 * of the Euler-Maruyama state, the latent log-volatility h the second, and the two noises are independent
 * (csrc/svf_math.hpp; the reference's SV_dense.py:203-223):
 *   y_t | y_t-1, h_t-1  ~  N(y_t-1 (1 + dt th0),  dt y_t-1^2 e^{h_t-1})
 *   h_t | h_t-1         ~  N(h_t-1 + dt (th1 - e^th2 h_t-1),  dt e^{2 th3})
 * The weight of a step depends on the particle's state before the move and the move does not depend on y_t, so
 * "weight on the pre-step state, resample, move" is the exactly fully adapted filter.
 *
 * vissm_sv_filter takes a VissmPfDesc with model = VISSM_MODEL_SV (anything else is refused); obs_std is ignored and
 * there is no obs_bin: every step is observed.  obs is the series y[0 .. T_total], T_total + 1 values; x_start
 * [K N] holds h at absolute step t0 (h_0 for t0 = 0), theta [K][4].  Geometry, N, Philox streams (AR's: n_stream = 1,
 * counter (ta / 4, 0, row); resampling on counter word 1 of row0 + k N), the integer pipeline, ll_inc, ess, loglik_in /
 * loglik, state_end, the traces, a NULL cloud, the death of a filter at W = 0 and chaining are vissm_particle_filter's.
 * Step ta = t0 + t:
 *   logw_i = -1/2 log 2 pi - log(sqrt(dt) |y[ta]|) - h_i / 2 - 1/2 r^2 / (dt y[ta]^2 e^{h_i}),
 *            r = y[ta + 1] - y[ta] - dt th0 y[ta];  -inf for a dead particle (h not finite)
 *   m, q_i, W, ll_inc, ess, U, tau_j, anc[j] from these as in vissm_particle_filter
 *   slot j takes h of particle anc[j] and moves it with the normal of its own row: the second coordinate of
 *   vissm_sde_simulate's SV step, bit for bit.
 * cloud [K N][1][H]: column t holds h after the move, an equally weighted sample of p(h_ta+1 | y_0:ta+1, theta).
 * loglik estimates log p(y_1:T | y_0, h_0, theta).  A y[ta] of 0 makes every weight NaN and kills the filter.
 * Refused by host arithmetic: a null descriptor or pointer, N not one of the five, negative shapes, t0 + H > T_total,
 * t0 + H >= 2^31, K N >= 2^31, dt not positive and finite.  Bitwise reproducible; filter k's bits depend on (seed,
 * row0 + k N, theta_k, N, y) only.  vissm_sv_filter_lds_bytes: the LDS one block declares (0 = bad N).
 *
 * vissm_sv_smooth is vissm_particle_smooth over that cloud (VissmPsDesc with model = VISSM_MODEL_SV; the same
 * geometry, M, selection on counter word 2, terminal rule, NaN propagation, x_first / x_next chaining, idx and
 * q_trace).  Column c (absolute ca = t0 + c) holds h_ca+1, and y_ca+2 depends on it, so the backward weight is not
 * the transition alone: for a trajectory whose next state is xt
 *   logw_i = log f(xt | h_i) + logw of h_i for (y[ca + 1], y[ca + 2]), less a constant of theta and dt.
 * It therefore takes obs and T_total as well, and refuses t0 + H + (x_next ? 1 : 0) > T_total: every column with a
 * next state reads y[ca + 2].  vissm_sv_smooth_lds_bytes: the LDS one block declares (0 = bad N or M).
 * ------------------------------------------------------------------------- */
int32_t vissm_sv_filter_lds_bytes(int32_t N);
int vissm_sv_filter(const VissmPfDesc* d, uint64_t seed, uint64_t row0,
                    const float* theta /* [K][4] */, const float* x_start /* [K N] */,
                    const float* obs /* [T_total + 1] */,
                    const double* loglik_in /* [K] or NULL */, double* loglik /* [K] */,
                    float* ll_inc /* [K][H] */, float* ess /* [K][H] */, float* state_end /* [K N] */,
                    float* cloud /* [K N][1][H] or NULL */, uint64_t* q_trace /* [K][H][N] or NULL */,
                    int32_t* anc_trace /* [K][H][N] or NULL */, void* stream);

int32_t vissm_sv_smooth_lds_bytes(int32_t N, int32_t M);
int vissm_sv_smooth(const VissmPsDesc* d, uint64_t seed, uint64_t row0,
                    const float* theta /* [K][4] */, const float* cloud /* [K N][1][H], vissm_sv_filter's */,
                    const float* obs /* [T_total + 1] */, int32_t T_total,
                    const float* x_next /* [K M] or NULL: the target of column H - 1 */,
                    float* paths /* [K M][1][H] */, float* x_first /* [K M] */,
                    int32_t* idx /* [K M][H] or NULL */, uint64_t* q_trace /* [K][H][M][N] or NULL: tests only */,
                    void* stream);

/* ---------------------------------------------------------------------------
 * Particle marginal Metropolis-Hastings over theta (Andrieu, Doucet & Holenstein 2010): C random-walk chains whose
 * acceptance ratio holds vissm_particle_filter_adapted's unbiased estimate of p(y | theta), so each chain targets
 * p(theta | y) exactly for any N.  AR, LV and FHN; one block per chain, N particles (the filter's five sizes), the
 * chain's n_iter iterations inside one launch.  Chain c runs the absolute iterations i = it0 .. it0 + n_iter - 1; with
 * r = row0 + (i C + c) N (csrc/mh_math.hpp):
 *   words   philox4x32_10(ctr = (g, 2, lo32(r), hi32(r)), key = seed): g = 0, 1 -> Box-Muller (the base noise's) ->
 *           xi_0 .. xi_7, the first P used; g = 2 -> first word x, u = ((x >> 8) + 1/2) 2^-24.  The normals of the
 *           filter carry 0 in the second counter word and its resampling integers 1: the streams never meet.
 *   theta'_p = float(theta_p + sum_{j <= p} L_pj xi_j), summed in double in ascending j; prop_chol = L [P][P] fp32, lower
 *   lp(theta) = -1/2 sum_p ((theta_p - m_p) / s_p)^2 in double; prior [P][2] fp32 = (mean, sd) per parameter
 *   ll' = the loglik vissm_particle_filter_adapted gives for K = C, row0' = row0 + i C N, t0 = 0, H = T_total, theta_c =
 *           theta', every particle started at x_start [S]: the same rows, normals, weights and resampling integers
 *   accept iff log(u) < (ll' - ll) + (lp' - lp), in double, in this arrangement: a dead proposal (ll' = -inf) is
 *           rejected, a chain at ll = -inf accepts any finite proposal, and -inf against -inf (NaN) is rejected.
 * ll_cur [C] is required: the estimate that goes with theta_cur (vissm_particle_filter_adapted with cloud = NULL).
 *
 * theta_chain [C][n_iter][P], ll_chain [C][n_iter] and accept [C][n_iter] hold the state after each decision;
 * theta_end [C][P] and ll_end [C] the last one: a call with it0' = it0 + n_iter, theta_cur = theta_end and ll_cur =
 * ll_end continues bitwise.  Optional traces for tests, NULL in production: theta_prop [C][n_iter][P], ll_prop and logu
 * [C][n_iter].  No atomics, no workspace; two launches are bitwise equal, and chain c's bits depend on the block index
 * through r only.  Refused by host arithmetic (VISSM_EINVAL): SV, an unknown model, N not one of the five, C < 1,
 * n_iter < 0, it0 < 0, it0 + n_iter >= 2^31, T_total S >= 2^31, obs_std <= 0 or not finite, a null pointer.
 * vissm_pmmh_lds_bytes: the LDS one block declares, 8 N + 4 S N + 192 (host arithmetic; 0 = bad model or N).
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t model, C, N, n_iter, it0, T_total;
  float dt, obs_std;
} VissmPmmhDesc;

int32_t vissm_pmmh_lds_bytes(int32_t model, int32_t N);
int vissm_pmmh(const VissmPmmhDesc* d, uint64_t seed, uint64_t row0,
               const float* theta_cur /* [C][P] */, const double* ll_cur /* [C] */,
               const float* prop_chol /* [P][P] lower */, const float* prior /* [P][2] (mean, sd) */,
               const float* x_start /* [S] */, const float* obs /* [S][T_total] */,
               const float* obs_bin /* [S][T_total] */,
               float* theta_chain /* [C][n_iter][P] */, double* ll_chain /* [C][n_iter] */,
               int32_t* accept /* [C][n_iter] */, float* theta_end /* [C][P] */, double* ll_end /* [C] */,
               float* theta_prop /* [C][n_iter][P] or NULL */, double* ll_prop /* [C][n_iter] or NULL */,
               double* logu /* [C][n_iter] or NULL */, void* stream);

/* ---------------------------------------------------------------------------
 * Particle marginal Metropolis-Hastings over theta of the stochastic-volatility model, which vissm_pmmh refuses for
 * want of an obs_std / obs_bin observation model: the same chains around vissm_sv_filter's filter, which is exactly
 * fully adapted, so each chain targets p(theta | y) exactly for any N.  VissmPmmhDesc with model = VISSM_MODEL_SV
 * (anything else is refused), obs_std ignored; P = 4.  One block per chain, N particles (the filter's five sizes), the
 * chain's n_iter iterations inside one launch.  Chain c runs the absolute iterations i = it0 .. it0 + n_iter - 1; with
 * r = row0 + (i C + c) N (csrc/mh_math.hpp):
 *   words, theta', lp(theta) and the decision are vissm_pmmh's, unchanged, with P = 4: the proposal's and the
 *           uniform's Philox blocks carry 2 in the second counter word, the filter's normals 0 and its resampling
 *           integers 1
 *   ll' = the loglik vissm_sv_filter gives for K = C, row0' = row0 + i C N, t0 = 0, H = T_total, theta_c = theta',
 *           every particle started at h_start[0] (not finite: the quiet NaN, a dead filter), over the series obs of
 *           T_total + 1 values: the same rows, normals, weights and resampling integers.  A filter that dies (W = 0; a
 *           zero in y[0 .. T_total - 1] kills it through NaN weights) gives ll' = -inf.
 *   accept iff log(u) < (ll' - ll) + (lp' - lp), in double: vissm_pmmh's rule and its -inf and NaN cases.
 * ll_cur [C] is required: the estimate that goes with theta_cur (vissm_sv_filter with cloud = NULL).
 *
 * Outputs, chaining through theta_end / ll_end and it0, the optional traces and reproducibility are vissm_pmmh's.  No
 * atomics, no workspace; two launches are bitwise equal.  Refused by host arithmetic (VISSM_EINVAL): a null
 * descriptor, a model other than SV, N not one of the five, C < 1, n_iter < 0, it0 < 0, it0 + n_iter >= 2^31,
 * T_total < 0 or >= 2^31 - 1, dt not positive and finite, a null pointer (obs may be NULL only if T_total = 0;
 * theta_chain, ll_chain and accept only if n_iter = 0).
 * vissm_sv_pmmh_lds_bytes: the LDS one block declares, 8 N + 4 N + 192 (host arithmetic; 0 = bad N).
 * ------------------------------------------------------------------------- */
int32_t vissm_sv_pmmh_lds_bytes(int32_t N);
int vissm_sv_pmmh(const VissmPmmhDesc* d, uint64_t seed, uint64_t row0,
                  const float* theta_cur /* [C][4] */, const double* ll_cur /* [C] */,
                  const float* prop_chol /* [4][4] lower */, const float* prior /* [4][2] (mean, sd) */,
                  const float* h_start /* [1]: h at step 0, every particle starts there */,
                  const float* obs /* y[0 .. T_total]: T_total + 1 values */,
                  float* theta_chain /* [C][n_iter][4] */, double* ll_chain /* [C][n_iter] */,
                  int32_t* accept /* [C][n_iter] */, float* theta_end /* [C][4] */, double* ll_end /* [C] */,
                  float* theta_prop /* [C][n_iter][4] or NULL */, double* ll_prop /* [C][n_iter] or NULL */,
                  double* logu /* [C][n_iter] or NULL */, void* stream);

/* ---------------------------------------------------------------------------
 * Adaptive particle marginal Metropolis-Hastings: vissm_pmmh / vissm_sv_pmmh with a proposal factor per chain that
 * the chain learns itself (robust adaptive Metropolis, Vihola 2012) while its absolute iteration i is below adapt_end,
 * and keeps frozen from adapt_end on.  The draws after adapt_end come from an ordinary fixed-proposal chain, which
 * targets p(theta | y) exactly; those before are a burn-in.  Everything the twins' blocks state holds unchanged: the
 * rows, the words, theta' (with L = the chain's factor of that iteration), lp, ll', the decision, the outputs and the
 * refusals.  chol_in [C][P][P] fp32 holds one lower factor per chain (the strict upper part is ignored).  After the
 * decision of an iteration i < adapt_end (csrc/mh_math.hpp, all in double):
 *   alpha  = 0 if r is NaN, 1 if r >= 0, else exp(r), with r = (ll' - ll) + (lp' - lp) of the state before the decision
 *            (a dead proposal gives 0, a chain at -inf meeting a finite proposal 1)
 *   eta    = min(1, P (i + 1)^-gamma),  d = eta (alpha - target_accept),  n2 = sum_{j < P} xi_j^2 (ascending j)
 *   skip   L is unchanged if !(n2 > 0), d == 0 or d is not finite
 *   v_p    = (sum_{j <= p} L_pj xi_j) sqrt(|d| / n2) (ascending j from 0.0),  sgn = the sign of d
 *   pass   for k = 0 .. P - 1:  r2 = L_kk^2 + sgn v_k^2 (L is unchanged if !(L_kk > 0) or !(r2 > 0));  rho = sqrt(r2),
 *            c = rho / L_kk, t = v_k / L_kk, L_kk = rho;  for i > k: L_ik = (L_ik + sgn t v_i) / c, then
 *            v_i = c v_i - t L_ik with the new L_ik
 *   round  every entry to fp32; if one is not finite or a diagonal entry is <= 0, L is unchanged as a whole
 * so L' L'^T = L (I + d xi xi^T / |xi|^2) L^T up to the fp32 rounding of the factor, positive definite as |d| < 1.
 * The factor is fp32 after every update: a frozen chain is bit for bit the twin's chain with prop_chol = its factor,
 * and adapt_end = 0 with every chain's factor equal is the twin.
 *
 * chol_end [C][P][P] is the factor after the last iteration (the strict upper part written 0): a call with it0' = it0 +
 * n_iter, theta_cur = theta_end, ll_cur = ll_end, chol_in = chol_end and the same adapt_end, target_accept and gamma
 * continues bitwise, across adapt_end too.  Optional traces for tests, NULL in production, beside the twins':
 * xi_trace [C][n_iter][8] fp32 the iteration's normals as the device drew them; alpha_trace and eta_trace [C][n_iter]
 * double (eta = 0 from adapt_end on); chol_trace [C][n_iter][P][P] fp32 the factor after the iteration.  The factor
 * lives in LDS and thread 0 updates it; no atomics, no workspace, nothing crosses blocks: chain c's bits depend on the
 * block index through r only.  Refused by host arithmetic (VISSM_EINVAL): what the twin refuses, adapt_end < 0,
 * target_accept outside (0, 1), gamma outside (0, 1] (a NaN is outside), a null chol_in or chol_end.
 * vissm_pmmh_adaptive_lds_bytes / vissm_sv_pmmh_adaptive_lds_bytes: the LDS one block declares, the twin's +
 * 8 (P P + 2 P) (the update's doubles) + 8 ceil(P P / 2) (the factor, in whole doubles): 8 N + 4 S N + 192 + 160 for
 * P = 3, + 256 for P = 4, + 384 for P = 5, and 8 N + 4 N + 192 + 256 for SV (host arithmetic; 0 = bad model or N).
 * ------------------------------------------------------------------------- */
int32_t vissm_pmmh_adaptive_lds_bytes(int32_t model, int32_t N);
int vissm_pmmh_adaptive(const VissmPmmhDesc* d, uint64_t seed, uint64_t row0,
                        const float* theta_cur /* [C][P] */, const double* ll_cur /* [C] */,
                        const float* chol_in /* [C][P][P] lower */, const float* prior /* [P][2] (mean, sd) */,
                        const float* x_start /* [S] */, const float* obs /* [S][T_total] */,
                        const float* obs_bin /* [S][T_total] */,
                        int32_t adapt_end, double target_accept, double gamma,
                        float* theta_chain /* [C][n_iter][P] */, double* ll_chain /* [C][n_iter] */,
                        int32_t* accept /* [C][n_iter] */, float* theta_end /* [C][P] */, double* ll_end /* [C] */,
                        float* chol_end /* [C][P][P] */,
                        float* theta_prop /* [C][n_iter][P] or NULL */, double* ll_prop /* [C][n_iter] or NULL */,
                        double* logu /* [C][n_iter] or NULL */, float* xi_trace /* [C][n_iter][8] or NULL */,
                        double* alpha_trace /* [C][n_iter] or NULL */, double* eta_trace /* [C][n_iter] or NULL */,
                        float* chol_trace /* [C][n_iter][P][P] or NULL */, void* stream);

int32_t vissm_sv_pmmh_adaptive_lds_bytes(int32_t N);
int vissm_sv_pmmh_adaptive(const VissmPmmhDesc* d, uint64_t seed, uint64_t row0,
                           const float* theta_cur /* [C][4] */, const double* ll_cur /* [C] */,
                           const float* chol_in /* [C][4][4] lower */, const float* prior /* [4][2] (mean, sd) */,
                           const float* h_start /* [1] */, const float* obs /* y[0 .. T_total] */,
                           int32_t adapt_end, double target_accept, double gamma,
                           float* theta_chain /* [C][n_iter][4] */, double* ll_chain /* [C][n_iter] */,
                           int32_t* accept /* [C][n_iter] */, float* theta_end /* [C][4] */, double* ll_end /* [C] */,
                           float* chol_end /* [C][4][4] */,
                           float* theta_prop /* [C][n_iter][4] or NULL */, double* ll_prop /* [C][n_iter] or NULL */,
                           double* logu /* [C][n_iter] or NULL */, float* xi_trace /* [C][n_iter][8] or NULL */,
                           double* alpha_trace /* [C][n_iter] or NULL */, double* eta_trace /* [C][n_iter] or NULL */,
                           float* chol_trace /* [C][n_iter][4][4] or NULL */, void* stream);

/* ---------------------------------------------------------------------------
 * Correlated pseudo-marginal Metropolis-Hastings for the stochastic-volatility model (Deligiannidis, Doucet & Pitt
 * 2018; csrc/cpm_math.hpp, csrc/sv_sorted.hip).  The chain carries the filter's random numbers as part of its state,
 * proposes them by u' = rho u + sqrt(1 - rho^2) eps and resamples in sorted order, so that the noise of ll' - ll falls
 * by an order of magnitude at the same N; it still targets p(theta | y) exactly.
 *
 * The auxiliary state of one filter of N particles over T = T_total steps, G = ceil(T / 4):
 *   aux_n [G][N][4] fp32  the move normals: entry (t, j) at group t / 4, slot j, word t % 4 (16-byte aligned; the tail
 *                         words of the last group are written 0 and never read)
 *   aux_r [T] fp32        the resampling normals
 *
 * vissm_sv_filter_sorted: K filters, VissmPfDesc with model = VISSM_MODEL_SV, t0 = 0 and H = T_total (anything else is
 * refused; there is no chaining in time), geometry and N as vissm_sv_filter.  theta [K][4], x_start [K N], obs
 * [T + 1], aux_n [K][G][N][4], aux_r [K][T].  Step ta:
 *   the N pre-step states are sorted ascending by key(h) = bits ^ 0x80000000 (sign clear) or ~bits (sign set), anything
 *   not finite 0xFFFFFFFF: position j holds h_(j), -0 before +0, dead particles (the quiet NaN) last;
 *   logw_j of h_(j), m, q_j, W, ll_inc, tau_j and anc[j] as in vissm_sv_filter, with
 *   U = min(2^24 - 1, floor(Phi(aux_r[ta]) 2^24)), Phi(x) = erfc(-x / sqrt 2) / 2 in double;
 *   position j takes h_(anc[j]) and moves it with the normal aux_n(ta, j).
 * W = 0 kills the filter (loglik = -inf, NaN after).  loglik [K] double, ll_inc [K][T].  Optional traces for tests,
 * NULL in production: cloud [K][T][N] (h after the move, in slot order), sorted_trace [K][T][N] (the pre-step states as
 * sorted), q_trace [K][T][N] uint64, anc_trace [K][T][N] int32, u_trace [K][T] uint32.  No random numbers are drawn, no
 * atomics: bitwise reproducible, and filter k's bits depend on (theta_k, its aux, N, y) only.
 * vissm_sv_filter_sorted_lds_bytes: 8 N + 4 N + 192 + (N > 64: 8 N for the sort's exchanges, else 4); 0 = bad N.
 *
 * vissm_sv_cpmmh: vissm_sv_pmmh_adaptive's chains (adapt_end = 0: fixed proposals from chol_in) around that filter.
 * A chain owns two halves of aux, aux_n [C][2][G][N][4] and aux_r [C][2][T]; aux_sel [C] int32 (0 or 1) says which half
 * belongs to the chain's current state (theta_cur, ll_cur).  All three are read and written.  Iteration i of chain c,
 * r = row0 + (i C + c) N:
 *   theta', lp', log u and the decision with its -inf and NaN cases are vissm_sv_pmmh's (counter word 2 of row r);
 *   un'(ta, j) = cn(un(ta, j), eps), eps the normal vissm_sv_pmmh's lane j consumes at step ta (row r + j, entry ta,
 *   counter word 0);  ur'(ta) = cn(ur(ta), eps_r), eps_r the first Box-Muller output of the Philox block
 *   (ta, 1, lo32(r), hi32(r));  cn(u, e) = fl32(fl32(rho u) + fl32(sqrt(1 - rho^2) e)), the root rounded once from double;
 *   the proposal's aux is written to the half aux_sel does not name;
 *   ll' = vissm_sv_filter_sorted's loglik on (theta', every particle at h_start[0], un', ur'), bit for bit;
 *   accept: theta, ll and lp are taken and aux_sel[c] ^= 1.  Nothing is copied.
 * A filter that dies leaves the rest of its half unwritten; a dead proposal is always rejected.  Outputs, traces,
 * the adaptation, chol_end and chaining (with the same aux tensors) are vissm_sv_pmmh_adaptive's.  Refused by host
 * arithmetic: what that entry refuses, rho outside [0, 1) (a NaN is outside), a null or misaligned aux pointer.
 * vissm_sv_cpmmh_lds_bytes: the filter's + 4 N + 256; 0 = bad N.
 * ------------------------------------------------------------------------- */
int32_t vissm_sv_filter_sorted_lds_bytes(int32_t N);
int vissm_sv_filter_sorted(const VissmPfDesc* d, const float* theta /* [K][4] */, const float* x_start /* [K N] */,
                           const float* obs /* [T_total + 1] */, const float* aux_n /* [K][G][N][4] */,
                           const float* aux_r /* [K][T] */, double* loglik /* [K] */, float* ll_inc /* [K][T] */,
                           float* cloud /* [K][T][N] or NULL */, float* sorted_trace /* [K][T][N] or NULL */,
                           uint64_t* q_trace /* [K][T][N] or NULL */, int32_t* anc_trace /* [K][T][N] or NULL */,
                           uint32_t* u_trace /* [K][T] or NULL */, void* stream);

int32_t vissm_sv_cpmmh_lds_bytes(int32_t N);
int vissm_sv_cpmmh(const VissmPmmhDesc* d, uint64_t seed, uint64_t row0,
                   const float* theta_cur /* [C][4] */, const double* ll_cur /* [C] */,
                   const float* chol_in /* [C][4][4] lower */, const float* prior /* [4][2] (mean, sd) */,
                   const float* h_start /* [1] */, const float* obs /* y[0 .. T_total] */,
                   int32_t adapt_end, double target_accept, double gamma, float rho,
                   float* aux_n /* [C][2][G][N][4], in and out */, float* aux_r /* [C][2][T], in and out */,
                   int32_t* aux_sel /* [C], in and out */,
                   float* theta_chain /* [C][n_iter][4] */, double* ll_chain /* [C][n_iter] */,
                   int32_t* accept /* [C][n_iter] */, float* theta_end /* [C][4] */, double* ll_end /* [C] */,
                   float* chol_end /* [C][4][4] */,
                   float* theta_prop /* [C][n_iter][4] or NULL */, double* ll_prop /* [C][n_iter] or NULL */,
                   double* logu /* [C][n_iter] or NULL */, float* xi_trace /* [C][n_iter][8] or NULL */,
                   double* alpha_trace /* [C][n_iter] or NULL */, double* eta_trace /* [C][n_iter] or NULL */,
                   float* chol_trace /* [C][n_iter][4][4] or NULL */, void* stream);

/* ---------------------------------------------------------------------------
 * Opt-in kernel timing (for bench.py's live roofline): when enabled, the flow
 * entry points bracket their main kernel with hipEvents on the launch stream.
 * kind: VISSM_PROF_FLOW_FWD / VISSM_PROF_FLOW_BWD (flow kernels),
 * VISSM_PROF_ELBO_FWD / VISSM_PROF_ELBO_BWD (log-density kernels), VISSM_PROF_NORMAL
 * (base-noise kernel).  read() synchronises the
 * recorded events and returns the summed milliseconds and the launch count.
 * ------------------------------------------------------------------------- */
#define VISSM_PROF_FLOW_FWD 0
#define VISSM_PROF_FLOW_BWD 1
#define VISSM_PROF_ELBO_FWD 2
#define VISSM_PROF_ELBO_BWD 3
#define VISSM_PROF_NORMAL 4
/* the flow backward launches again, by variant (each launch is also counted in VISSM_PROF_FLOW_BWD):
 * without du (the first flow: its input is the base noise), with du (middle flows), and the last AR(1)
 * flow fused with its ELBO terms (vissm_flow_ar_elbo_fused) */
#define VISSM_PROF_FLOW_BWD_NODU 5
#define VISSM_PROF_FLOW_BWD_DU 6
#define VISSM_PROF_FLOW_FUSED 7
void vissm_profile_enable(int32_t on);
int vissm_profile_read(int32_t kind, double* total_ms, int64_t* count);
void vissm_profile_reset(void);
/* Summed algorithmic HBM bytes of the recorded launches of `kind` (the streaming kernels
 * state theirs: ELBO_FWD / ELBO_BWD / NORMAL; 0 for the flow kernels). */
int vissm_profile_bytes(int32_t kind, double* total_bytes);

#ifdef __cplusplus
}
#endif
#endif /* VISSM_H */
