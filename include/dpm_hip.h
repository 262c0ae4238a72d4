/*
 * dpm_hip.h -- C ABI of the MI355X-native DPM-Solver / DPM-Solver++ sampling engine.
 *
 * The reference (LuChengTHU/dpm-solver, dpm_solver_pytorch.py) has no FFI boundary: its "plugin
 * interface" is the Python API  NoiseScheduleVP / model_wrapper / DPM_Solver  (README.md:380).
 * This header is the boundary a host in any language binds to *under* that API; the Python
 * mirror in dpm_solver_amd/ is one such host (ctypes).
 *
 * Design:
 *   - every scalar of the noise schedule (alpha_t, sigma_t, lambda_t, h, r, phi_k) is computed
 *     ONCE on the host by the planner, in the reference's own fp32 operation order, and frozen
 *     into a list of `dpm_stage` records -- one per network evaluation;
 *   - the device runs exactly one fused streaming kernel per stage:
 *        raw network output(s) -> [CFG blend | classifier term] -> [x_start/v/score -> eps]
 *        -> [eps -> x0] -> [dynamic thresholding] -> exponential-integrator update
 *     reading the state x, the fresh output(s) and 0-2 cached model values, writing x_next and
 *     (if a later stage needs it) the new model value;
 *   - the library never allocates or frees user-visible device memory: every buffer is the
 *     caller's, every launch is asynchronous on the caller's HIP stream, nothing synchronises.
 *
 * Conventions: plain C types only.  Return value 0 = DPM_OK, negative = argument/state error
 * (dpm_last_error() has the text), positive = a hipError_t from the HIP runtime.  No function
 * throws or aborts.  Handles are immutable after creation and may be shared between threads.
 * `stream` is a hipStream_t passed as void* (NULL = the null stream).
 */
#ifndef DPM_HIP_H
#define DPM_HIP_H

#include <stddef.h>
#include <stdint.h>

/* The library is compiled with -fvisibility=hidden: DPM_API marks the entry points, which are then the ONLY symbols in its
   dynamic table (tests/test_capi_symbols.py compares `nm -D --defined-only` with this header name by name) -- no mangled
   internal can collide with a symbol of the host process or of a second library it links. */
#ifndef DPM_API
#define DPM_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* major*10000 + minor*100 + patch.  History: 100 rounds 1-2; 101 dpm_buffers / dpm_run_buffers gained the trailing
   `thr_hint` pointer; 102 dpm_cluster_timeout_poll, DPM_TUNE_THR_SPIN_LIMIT / _DEBUG_FAULT, DPM_ERR_FAULT retired;
   103 DPM_TUNE_BLOCK_THREADS, dpm_calib_launch kind 2 (no struct changed);
   200 (round 5) the measurement / tuning / experiment entry points left this header and the product library: dpm_tuning_*,
   dpm_calib_launch, dpm_prefetch_launch, dpm_resident_*, dpm_trace_*, dpm_stage_launch_timed and dpm_plan_run_timed are
   declared in include/dpm_lab.h and exported by the lab build only (libdpm_lab.so, the same sources with -DDPM_LAB=1);
   what a caller may legitimately choose per call travels in dpm_launch_opts (dpm_buffers.opts / dpm_run_buffers.opts);
   DPM_DTYPE_F64 (double-precision state, NoiseScheduleVP(dtype=torch.float64) callers).  The product library has no
   process-global mutable state: per-device contexts only (the chain of clustered launches, the diagnostics word).
   201 (round 6) dpm_add_noise_launch_f64 (double times on double tensors); -fvisibility=hidden + DPM_API: the dynamic symbol
   table is this header's functions and nothing else.
   202 dpm_launch_opts.per_request_stages (was reserved[0]): dpm_stage_launch_multi with one stage record per request --
   requests at different positions of different plans in one fused launch (continuous batching).
   203 DPM_ALGO_SDE_DPMSOLVERPP, DPM_F_NOISE and dpm_launch_opts.noise_seed_lo / _hi (were reserved[0..1]): SDE-DPM-Solver++
   with its Gaussian term generated inside the stage kernel (see "noise contract" below; no struct changed size).
   204 dpm_stage_launch_multi / dpm_plan_run_multi fuse DPM_F_NOISE stages too -- lockstep and per-request stages -- with the
   seed of every request taken from its own bs[r].opts (no entry point added, no struct changed).
   205 DPM_ALGO_UNIPC, DPM_SOLVER_UNIPC_BH1 / _BH2, DPM_FORM_UNIPC, DPM_F_UNIPC_DP / _P2, DPM_F_STORE_XC: UniPC sampling with
   the corrector of step i and the predictor of step i+1 in ONE stage launch (see DPM_FORM_UNIPC; no entry point added, no
   struct changed).
   206 dpm_stage_launch_multi with per-request stages fuses DPM_FORM_UNIPC stages too, at any position and next to first- and
   second-order stages (UniPC requests in continuous batching; no entry point added, no struct changed).
   207 dpm_launch_opts.fuse_shapes (was reserved[0]): dpm_stage_launch_multi with per-request stages fuses requests of
   DIFFERENT n and batch in one launch (a server's 512^2, 768^2 and 1024^2 latents side by side; no entry point added, no
   struct changed size).
   208 dpm_launch_opts.table_mode (was reserved[0]), DPM_TABLE_FILL / DPM_TABLE_LAUNCH, DPM_SIZEOF_TABLE_HEADER / _ROW:
   dpm_stage_launch_multi with per-request stages launches a group of MORE than 16 requests as ONE kernel whose per-request
   records are rows of a table in device memory (hundreds of single-image requests per tick; see "Table mode" at
   dpm_stage_launch_multi; no entry point added, no struct changed size).
   209 DPM_TABLE_NOISE (a flag on table_mode), dpm_buffers.noise_sample0 (was `reserved`), DPM_TABLE_NOISE_BYTES /
   DPM_SIZEOF_TABLE_NOISE: SDE stages in the table -- every fusable DPM_F_NOISE request owns a row and a noise record behind
   the rows, and a row may be ONE SAMPLE of a request whose noise the contract indexes over all of its samples (see "Table
   mode"; no entry point added, no struct changed size).
   210 DPM_TABLE_THRESH (a flag on table_mode): thresholded stages in the table -- every DPM_F_THRESH request whose sample fits
   one workgroup's LDS owns a row, a group of them is ONE cluster-free launch without a workspace (see "Table mode"; no entry
   point added, no struct changed, rows and records as in version 209).
   211 DPM_TABLE_BLEND (a flag on table_mode), DPM_TABLE_BLEND_BYTES / DPM_SIZEOF_TABLE_BLEND: mask-blend stages (DPM_F_BLEND,
   inpainting / DiffEdit) in the table -- every qualifying DPM_F_BLEND request owns a row and a blend record behind the rows,
   a group of them is ONE stage_kernel_table_blend launch (see "Table mode"; no entry point added, no struct changed size).
   212 DPM_F_CFG_RESCALE: classifier-free guidance with guidance rescale (Lin et al. 2023, section 3.4; diffusers'
   guidance_rescale) in ONE stage launch -- a kernel that owns a whole sample, takes the two per-sample standard deviations,
   then runs the usual prologue, update and stores (see DPM_F_CFG_RESCALE; no entry point added, no struct changed).
   213 DPM_TABLE_RESCALE (a flag on table_mode): guidance-rescale stages in the table -- every qualifying DPM_F_CFG_RESCALE
   request owns a row, a group of them is ONE stage_rescale_kernel_table launch, one workgroup per sample (see "Table mode"; no
   entry point added, no struct changed, rows and records as in version 211).
   214 DPM_F_CFG_APG: classifier-free guidance with adaptive projected guidance (Sadat et al. 2024; diffusers' APG guider) in
   ONE stage launch -- a kernel that owns a whole sample, splits the guidance direction of the two data predictions into its
   components parallel and orthogonal to the conditional one, damps the parallel one, caps the direction's norm and optionally
   carries a running average of it from stage to stage (see DPM_F_CFG_APG; no entry point added, no struct changed).
   215 DPM_TABLE_APG (a flag on table_mode), DPM_TABLE_APG_BYTES / DPM_SIZEOF_TABLE_APG: adaptive-projected-guidance stages in
   the table -- every qualifying DPM_F_CFG_APG request owns a row and an APG record behind the rows, a group of them is ONE
   stage_apg_kernel_table launch, one workgroup per sample; in such a call a request's running average is dpm_buffers.thr_hint
   (see "Table mode"; no entry point added, no struct changed size).
   216 DPM_F_CFG_ZSTAR: classifier-free guidance with the CFG-Zero* projection (Fan et al. 2025; diffusers'
   ClassifierFreeZeroStarGuidance, ComfyUI's CFGZeroStar) in ONE stage launch -- a kernel that owns a whole sample, takes the
   per-sample least-squares fit of the unconditional output to the conditional one, scales the unconditional output by it, then
   runs the usual blend, conversion, update and stores (see DPM_F_CFG_ZSTAR; no entry point added, no struct changed).
   217 DPM_TABLE_ZSTAR (a flag on table_mode): CFG-Zero* stages in the table -- every qualifying DPM_F_CFG_ZSTAR request owns a
   row, a group of them is ONE stage_zstar_kernel_table launch, one workgroup per sample (see "Table mode"; no entry point
   added, no struct changed, rows and records as in version 215: the kind has no record section).
   218 DPM_GUIDE_CFG2: guidance over TWO conditions -- three network outputs per evaluation (e0, e1 and g) blended in ONE stage
   launch, eps = (n1 + s1 * (n0 - n1)) + s2 * (n2 - n1) with s1 = cfg_scale and s2 = cg_scale (InstructPix2Pix's image and text
   scales, composable conditions): a streaming kernel of its own, stage_pair_kernel, one instantiation per dtype pair (see
   DPM_GUIDE_CFG2; no entry point added, no struct changed).  The planner and dpm_coef_prologue[_f64] accept the value.
   219 DPM_TABLE_PAIR (a flag on table_mode), DPM_TABLE_PAIR_BYTES / DPM_SIZEOF_TABLE_PAIR: two-condition stages in the table --
   every qualifying DPM_GUIDE_CFG2 request owns a row and a pair record behind the rows (the third network output, the third
   copy of x_out), a group of them is ONE stage_pair_kernel_table launch; in such a call a DPM_GUIDE_CFG2 request may carry
   x_out2, with the THIRD copy of x_out in dpm_buffers.thr_hint (see "Table mode"; no entry point added, no struct changed).
   220 DPM_F_CFG2_PERP: Perp-Neg guidance (Armandpour et al. 2023; ComfyUI's PerpNeg) on a DPM_GUIDE_CFG2 stage in ONE stage
   launch -- a kernel that owns a whole sample, takes the negative condition's direction perpendicular to the positive one's
   by a per-sample projection of the three raw outputs, then runs the usual conversion, update and stores (see
   DPM_F_CFG2_PERP; no entry point added, no struct changed).
   221 DPM_TABLE_PERP (a flag on table_mode): Perp-Neg stages in the table -- every qualifying DPM_F_CFG2_PERP request owns a row
   and a pair record (the record of version 219, in the same section), a group of them is ONE stage_perp_kernel_table launch, one
   workgroup per sample, which stores the state up to three times; in such a call a flagged DPM_GUIDE_CFG2 request may carry
   x_out2, with the THIRD copy of x_out in dpm_buffers.thr_hint (see "Table mode"; no entry point added, no struct changed, no
   dpm_sizeof index added).
   The structs grow at their END only.  A host MUST zero-initialise every struct it passes (memset / = {0}: new trailing
   fields then read as "absent") and SHOULD check at load time that dpm_version() >= the version it was built against and
   that dpm_sizeof(DPM_SIZEOF_*) == its own sizeof() -- a host compiled against an older header passes shorter structs,
   and the library would read past their end (examples/native_host.c and dpm_solver_amd/_lib.py do both checks). */
#define DPM_HIP_VERSION 221

/* ---- status --------------------------------------------------------------------------- */
enum {
  DPM_OK = 0,
  DPM_ERR_ARG = -1,         /* bad argument value (ValueError at the Python layer)            */
  DPM_ERR_UNSUPPORTED = -2, /* valid in the reference, not (yet) built here -- never silent   */
  DPM_ERR_ALIGN = -3,       /* a buffer is not aligned as the entry point requires (lab entry points only)   */
  DPM_ERR_NOMEM = -4,
  DPM_ERR_CALLBACK = -5,    /* the model callback of dpm_plan_run returned non-zero           */
  DPM_ERR_FAULT = -6        /* retired (version 102): a clustered thresholding launch whose wait on a peer
                               workgroup times out now recovers inside the kernel -- the workgroup computes
                               the sample's order statistics alone, results unchanged -- and no entry point
                               returns this code any more; see dpm_cluster_timeout_poll                      */
};

/* ---- enumerations (values are ABI) ----------------------------------------------------- */
enum { DPM_ALGO_DPMSOLVER = 0, DPM_ALGO_DPMSOLVERPP = 1,          /* algorithm_type, ref :342,:406 */
       DPM_ALGO_SDE_DPMSOLVERPP = 2 /* version 203: the stochastic multistep DPM-Solver++ ("DPM++ 2M SDE", diffusers'
                                       sde-dpmsolver++).  dpm_plan_create only (method multistep, order 1 or 2, fp32
                                       scalars, no thresholding); the per-update coefficient builders reject it */,
       DPM_ALGO_UNIPC = 3 /* version 205: UniPC (Zhao et al. 2023; diffusers' UniPCMultistepScheduler) in the data-prediction
                             form, predictor AND corrector.  dpm_plan_create only (method multistep, order 1 or 2, fp32
                             scalars, no thresholding; solver_type = DPM_SOLVER_UNIPC_BH1 / _BH2); the per-update coefficient
                             builders reject it.  The plan is the multistep DPM-Solver++ plan -- one stage per network
                             evaluation, same times and buffer roles -- with the step orders o_i = min(order, i, steps + 1 - i)
                             (lower_order_final; else min(order, i)) and stages 1 .. steps-1 of form DPM_FORM_UNIPC; every
                             scalar is evaluated in double and rounded once */ };
enum { DPM_SOLVER_DPMSOLVER = 0, DPM_SOLVER_TAYLOR = 1,           /* solver_type,    ref :611      */
       DPM_SOLVER_UNIPC_BH1 = 2, DPM_SOLVER_UNIPC_BH2 = 3 /* version 205, DPM_ALGO_UNIPC only: UniPC's B(h) = -h | expm1(-h) */ };
enum { DPM_METHOD_MULTISTEP = 0, DPM_METHOD_SINGLESTEP = 1, DPM_METHOD_SINGLESTEP_FIXED = 2 }; /* ref :1171,:1214 */
enum { DPM_SKIP_TIME_UNIFORM = 0, DPM_SKIP_LOGSNR = 1, DPM_SKIP_TIME_QUADRATIC = 2 };          /* ref :468-478    */
enum { DPM_MODEL_NOISE = 0, DPM_MODEL_X_START = 1, DPM_MODEL_V = 2, DPM_MODEL_SCORE = 3 };     /* ref :288-298    */
enum { DPM_GUIDE_NONE = 0, DPM_GUIDE_CFG = 1, DPM_GUIDE_CLASSIFIER = 2,                       /* ref :313-330    */
       DPM_GUIDE_CFG2 = 3 /* version 218: classifier-free guidance over TWO conditions, three network outputs per evaluation.
                             Operands, all of the eps dtype and all following eps_stride (0 or P = n / batch only):
                               e0 = the raw output under the first condition, e1 = the unconditional raw output,
                               g  = the raw output under the second condition.
                             Scalars: s1 = dpm_stage.cfg_scale, s2 = dpm_stage.cg_scale (the planner writes 0 there under this
                             guidance; the caller overwrites it, as it does with phi under DPM_F_CFG_RESCALE).
                             Arithmetic, fp32 on the exactly widened outputs, one rounding per operation, no fused multiply-add:
                               n_k = noise prediction of the raw output o_k (x_start / v / score conversion of the stage's model
                                     type on xe), k = 0, 1, 2
                               d0 = n0 - n1;  d2 = n2 - n1;  eps = (n1 + s1 * d0) + s2 * d2
                             then DPM_F_TO_X0, the update form (LIN1 .. DENOISE, DPM_F_BASE_HIST included), DPM_F_STORE_M and the
                             stores as under any other guidance.  Nothing is rounded to the network's dtype, not even for a 2-byte
                             noise-prediction network, and the model values are never half-precision tensors under it: every
                             difference of two model values is an fp32 operation.  InstructPix2Pix's e_u + s_I (e_I - e_u) +
                             s_T (e_IT - e_I) is e0 = e_IT, g = e_I, s1 = s_T, s2 = s_I - s_T; composable conditions e_u +
                             s (e_c - e_u) + s' (e_c' - e_u) are s1 = s, s2 = s'.  With FP32 outputs the result is DPM_GUIDE_CFG's
                             bit for bit when s2 == 0, and when g == e1 (d2 = 0, and adding s2 * 0 changes no bit).  With a
                             2-byte noise-prediction network neither holds: DPM_GUIDE_CFG rounds its blend to that dtype, this
                             guidance does not.
                             DPM_ERR_ARG: e1 or g is NULL; s1 or s2 is not finite; one of DPM_F_CFG_RESCALE / _APG / _ZSTAR
                             (they are valid under DPM_GUIDE_CFG only); an unknown form.
                             DPM_ERR_UNSUPPORTED (this version): DPM_F_THRESH, DPM_F_BLEND, DPM_F_NOISE, DPM_F_USER_X0;
                             DPM_FORM_UNIPC; a non-NULL x_out2; a double state; eps_stride other than 0 or P; device-resident
                             coefficients.  No output byte is written in any error case.  One streaming kernel
                             (stage_pair_kernel: 2048-element tiles, 16-byte accesses where n is a multiple of 8 and every
                             operand is 16-byte aligned, else one element per lane); such a stage runs on its own in a
                             multi-request launch, in every mode of dpm_stage_launch_multi.  dpm_plan_create and
                             dpm_coef_prologue[_f64] treat the value as DPM_GUIDE_CFG for cfg_scale */ };
enum { DPM_DTYPE_F32 = 0, DPM_DTYPE_F16 = 1, DPM_DTYPE_BF16 = 2,
       DPM_DTYPE_F64 = 3 /* state AND network output in double, double arithmetic: the reference run on x.double()
                            (ref :14, :105-107); one run-time dispatched kernel, not a performance path */ };
enum { DPM_EVAL_LOG_ALPHA = 0, DPM_EVAL_ALPHA = 1, DPM_EVAL_STD = 2, DPM_EVAL_LAMBDA = 3, DPM_EVAL_INV_LAMBDA = 4 };

/* update forms.  `mn` = model value produced by this stage's prologue, h1/h2 = cached values.  */
enum {
  DPM_FORM_LIN1 = 0,    /* out = cx*x - c0*mn                                         (ref :573,:585)        */
  DPM_FORM_TWO = 1,     /* D = k0*(mn-h1); out = (cx*x - c0*P) - c1*D, P = BASE_HIST ? h1 : mn
                           (ref :636-646,:659-669,:728-739,:767-778,:827-851)                               */
  DPM_FORM_MS3 = 2,     /* multistep third order (ref :879-903)                                              */
  DPM_FORM_SS3T = 3,    /* singlestep third order, 'taylor' final combination (ref :741-750,:780-789)        */
  DPM_FORM_DENOISE = 4, /* out = mn  (denoise_to_zero, ref :541-545,:1235-1237)                              */
  DPM_FORM_UNIPC = 5,   /* version 205.  UniPC stage i (1 <= i < steps): the corrector of step i, then the predictor of step
                           i+1 on the corrected state, which never leaves the registers.  x = x_i^p (the state the network
                           saw: x = xe), mn = m_i, h1 = m_{i-1}, h2 = m_{i-2} (DPM_F_UNIPC_DP only):
                             d1 = mn - h1
                             xc = x + (c2 * (k[2] * (h2 - h1)) - k[1] * d1)     with DPM_F_UNIPC_DP (second-order corrector)
                             xc = x - k[1] * d1                                  without         (first-order corrector)
                             out = (cx * xc - c0 * mn) - c1 * (k[0] * d1)        with DPM_F_UNIPC_P2 (second-order predictor)
                             out = cx * xc - c0 * mn                             without         (first-order predictor)
                           fp32, one rounding per operation, one rounding of out (and of xc, DPM_F_STORE_XC) to the state dtype.
                           With h = lambda_i - lambda_{i-1}, B = -h (bh1) | expm1(-h) (bh2), r = (lambda_{i-2} - lambda_{i-1}) / h
                           and rho^c the solution of [[1, 1], [r, 1]] rho = [b_1, b_2] (rho^c = [1/2] in first order):
                             c2 = alpha_i B (1/2 - rho^c_1), k[1] = alpha_i B rho^c_last, k[2] = 1 / r -- the published corrector
                             x_i = xbar_i - alpha_i B (rho^c_1 D_p + rho^c_2 (m_i - m_{i-1})) minus the published predictor
                             x_i^p = xbar_i - alpha_i B D_p / 2, D_p = (m_{i-2} - m_{i-1}) / r;
                             cx, c0, c1, k[0]: the DPM_FORM_LIN1 / _TWO scalars of step i+1 with c1 = alpha_{i+1} B_{i+1} / 2.
                           No thresholding, mask blend, noise, double state or device-resident coefficients: DPM_ERR_UNSUPPORTED */
  DPM_FORM_COUNT = 6
};

/* dpm_stage.flags */
#define DPM_F_TO_X0 1u      /* prologue converts eps -> x0 = (xe - sigma*eps)/alpha   (ref :439)              */
#define DPM_F_STORE_M 2u    /* write mn to m_out (a later stage reads it as h1/h2)                            */
#define DPM_F_BASE_HIST 4u  /* FORM_TWO: first-order term uses h1 (singlestep) instead of mn (multistep)      */
#define DPM_F_THRESH 8u     /* dynamic thresholding of x0 (ref :416-425)                                      */
#define DPM_F_USER_X0 16u   /* host applies a callable correcting_x0_fn: stage is split by the host shim       */
#define DPM_F_BLEND 32u     /* epilogue: x_out <- x_out*mask + (1-mask)*(blend_alpha*blend_a + blend_sigma*blend_b),
                               the mask blend DiffEdit / inpainting callers run as correcting_xt_fn after every
                               update (scripts/diffedit_inpaint.ipynb cell 6; hook: ref :1180,:1188,:1203,:1229)     */
#define DPM_F_NOISE 64u     /* version 203, forms LIN1 / TWO only: out += c2 * z before the store rounding (and before a
                               DPM_F_BLEND epilogue), z the standard normal of the noise contract below with counter
                               dpm_stage.index and the seed of dpm_launch_opts.noise_seed_lo / _hi.  With thresholding,
                               another form, a double state or device-resident coefficients: DPM_ERR_ARG.
   Noise contract.  z of element i -- i = index in the flat, contiguous [B, C, H, W] order of the state -- depends on (seed,
   stage index, i) only: not on the launch shape, tile mapping, dtype pair, kernel or the batch around it.
     key = (seed lo, seed hi), counter = ((i >> 2) lo, (i >> 2) hi, stage index, 0); r[0..3] = Philox4x32-10(key, counter)
     (Random123; zero key and counter give 6627e8d5 e169c58d bc57ac4c 9b00dbd8);
     u(r) = ((r >> 9) + 0.5) * 2^-23: the 23 high bits, centred -- exact in fp32 and inside (0, 1) (24 bits + 0.5 would need
     25 significant bits);  element i takes the pair p = (i & 3) >> 1:
     z = sqrt(-2 ln u(r[2p])) * (i even ? cos : sin)(2 pi u(r[2p + 1]))
     in fp32 (logf, sqrtf, the hardware sine / cosine of u in revolutions), the same device function on every route. */

#define DPM_F_UNIPC_DP 128u  /* version 205, DPM_FORM_UNIPC: the corrector is second order (reads h2)                       */
#define DPM_F_UNIPC_P2 256u  /* DPM_FORM_UNIPC: the predictor of the next step is second order                              */
#define DPM_F_STORE_XC 512u  /* DPM_FORM_UNIPC: dpm_buffers.x_out2 receives the CORRECTED state xc (the solver state x_i a
                                caller of return_intermediate wants) instead of a second copy of x_out; never set by the
                                planner.  Such a stage runs on its own in a multi-request launch                          */

#define DPM_F_CFG_RESCALE 1024u /* version 212, with guidance == DPM_GUIDE_CFG only (else DPM_ERR_ARG); never set by the planner.
                                  Guidance rescale: the guided output is rescaled so that its per-sample standard deviation
                                  matches the conditional output's, and blended with the un-rescaled one by phi.  With the flag
                                  dpm_stage.cg_scale carries phi in (0, 1] (under CFG the planner writes that field and nothing
                                  reads it; the caller overwrites it).  For each sample b of the launch, P = n / batch elements,
                                  s = cfg_scale:
                                    o_c, o_u = e0, e1 of the sample as fp32             (the RAW outputs: before any conversion)
                                    g   = o_u + s * (o_c - o_u)      fp32, one rounding per operation; a 2-byte noise-prediction
                                                                     network: each of the three operations rounded through the
                                                                     network's dtype, as the flag-less blend is
                                    d_c = (double)o_c - (double)o_c[0];  d_g = (double)g - (double)g[0]     (the sample's first element)
                                    S1 = sum d, S2 = sum d * d       in double, no fused multiply-add, any summation order
                                    var = max((S2 - S1 * S1 / P) / (P - 1), 0);  std = sqrt(var)     in double (unbiased: torch.std)
                                    f   = (float)(std_c / std_g)     one double division, one rounding to fp32
                                    r   = phi * (g * f) + (1.f - phi) * g               fp32, one rounding per operation
                                    eps = noise prediction of the raw output r (x_start / v / score conversion), then
                                          DPM_F_TO_X0, the update form and the stores as without the flag, all fp32: r is
                                          an fp32 value whatever the network's dtype, nothing after the blend is rounded to it
                                  The statistics are those of the raw outputs (the paper, diffusers): for an x_start / v / score
                                  network the blend therefore precedes the conversion, which it follows without the flag.  A
                                  sample with std_g == 0 gets what IEEE gives (inf or NaN in every element), like torch.
                                  DPM_ERR_ARG: P < 2 (an empty batch, n == 0, is DPM_OK and launches nothing, as for every
                                  stage); phi outside (0, 1] or NaN; the flag without DPM_GUIDE_CFG; an unknown form.
                                  DPM_ERR_UNSUPPORTED (this version): DPM_F_THRESH, DPM_F_BLEND, DPM_F_NOISE; DPM_FORM_UNIPC; a
                                  double state; eps_stride other than 0 or P; device-resident coefficients.  No output byte is
                                  written in any error case.  One workgroup per sample (stage_rescale_kernel); such a stage runs
                                  on its own in a multi-request launch, in every mode of dpm_stage_launch_multi */

#define DPM_F_CFG_APG 2048u /* version 214, with guidance == DPM_GUIDE_CFG only (else DPM_ERR_ARG); never set by the planner.
                               Adaptive projected guidance (Sadat et al. 2024): the guidance direction -- the difference of the
                               conditional and the unconditional DATA prediction -- is capped in norm per sample, split into its
                               components parallel and orthogonal to the conditional prediction, the parallel one damped by eta,
                               and optionally smoothed over the stages by a (negative) momentum.  The flag reuses fields nothing
                               else reads under it: dpm_stage.cg_scale carries eta in [0, 1], dpm_stage.thr_ratio the norm
                               threshold r >= 0 (0 = off), dpm_stage.thr_max the momentum beta in (-1, 1) (0 = off), and with
                               beta != 0 dpm_buffers.workspace the RUNNING AVERAGE: n fp32 values in the state's flat order, read
                               and written in place (the caller zero-fills it where a trajectory starts).  In a table call that
                               carries DPM_TABLE_APG (version 215) the running average is dpm_buffers.thr_hint instead, for EVERY
                               request of the call, and workspace is not read for it: see "Table mode".  For each sample of
                               the launch, P = n / batch elements, s = cfg_scale:
                                 c = x0 of the conditional output e0, u = x0 of the unconditional output e1: the noise
                                     prediction of the raw output on xe (x_start / v / score conversion), then
                                     (xe - sigma_e * eps) / alpha_e -- operation for operation the model value of a flag-less
                                     data-prediction stage; raw outputs are widened to fp32 on load, nothing after that is
                                     rounded to the network's dtype
                                 d = c - u                                               fp32
                                 beta != 0:  a = d + beta * a  (fp32, one rounding per operation, no fused multiply-add);
                                             a is stored;  d = a
                                 S_dd = sum d*d, S_dc = sum d*c, S_cc = sum c*c          products and sums in double, any order
                                 sc64 = r > 0 ? (t < 1 ? t : 1) : 1,  t = (double)r / sqrt(S_dd)      double
                                 sc = (float)sc64;  q = (float)((sc64 * S_dc) / S_cc)    one rounding each
                                 dn = sc * d;  par = q * c;  upd = (dn - par) + eta * par          fp32, one rounding per operation
                                 mn = c + (s - 1.f) * upd                                the guided data prediction
                                 then the update form, DPM_F_STORE_M and the stores as without the flag
                               A degenerate sample (S_cc == 0) gets what IEEE gives.  With eta = 1, r = 0 and beta = 0 the result
                               is classifier-free guidance up to rounding.
                               DPM_ERR_ARG: the flag without DPM_GUIDE_CFG; eta, r or beta out of range or NaN; beta != 0 with a
                               null workspace (a null thr_hint in a DPM_TABLE_APG call); an unknown form; P < 1 (an empty batch, n == 0, is DPM_OK and launches nothing).
                               DPM_ERR_UNSUPPORTED (this version): the flag without DPM_F_TO_X0 (it is defined on the data
                               prediction); together with DPM_F_CFG_RESCALE, DPM_F_THRESH, DPM_F_BLEND or DPM_F_NOISE;
                               DPM_FORM_UNIPC; a double state; eps_stride other than 0 or P; device-resident coefficients.  No
                               output byte is written in any error case, the running average neither.  One workgroup per
                               sample (stage_apg_kernel); such a stage runs on its own in a multi-request launch, in every mode
                               of dpm_stage_launch_multi (in a table call it cannot be st[0] with beta != 0: bs[0].workspace is
                               the table there -- DPM_ERR_ARG) */

#define DPM_F_CFG_ZSTAR 4096u /* version 216, with guidance == DPM_GUIDE_CFG only (else DPM_ERR_ARG); never set by the planner.
                                 CFG-Zero* (Fan et al. 2025): before the blend, the unconditional output is scaled by its
                                 per-sample least-squares fit to the conditional one.  The flag reads no field beyond cfg_scale.
                                 For each sample of the launch, with P = n / batch elements and s = cfg_scale:
                                   o_c, o_u = e0, e1 of the sample widened to fp32     (the RAW outputs, before any conversion --
                                                                                        as under DPM_F_CFG_RESCALE)
                                   S_cu = sum (double)o_c * (double)o_u     products exact in double; sums in double, any order
                                   S_uu = sum (double)o_u * (double)o_u
                                   a    = (float)(S_cu / (S_uu + 1e-8))     one double addition, one double division, one rounding
                                                                            to fp32
                                   u    = a * o_u                           fp32, one rounding per operation, no fused multiply-add
                                   g    = u + s * (o_c - u)                 fp32, one rounding per operation, no fused multiply-add
                                   eps  = noise prediction of the raw output g (x_start / v / score conversion), then
                                          DPM_F_TO_X0, the update form, DPM_F_STORE_M, x_out2 and the stores as without the flag,
                                          all fp32
                                 g is an fp32 value whatever the network's dtype: nothing after the loads is rounded to the
                                 network's dtype, not even for a 2-byte noise-prediction network.  S_uu == 0 gives a = 0 and
                                 g = s * o_c: defined behaviour, not an IEEE accident.  The paper's "zero-init" (a zero velocity
                                 in the first steps) is not part of the flag: it is defined for flow-matching velocities and has
                                 no counterpart for a VP noise prediction.  Both algorithm types, with or without DPM_F_TO_X0.
                                 DPM_ERR_ARG: the flag without DPM_GUIDE_CFG; P < 1 (an empty batch, n == 0, is DPM_OK and
                                 launches nothing); an unknown form.
                                 DPM_ERR_UNSUPPORTED (this version): together with DPM_F_CFG_RESCALE, DPM_F_CFG_APG, DPM_F_THRESH,
                                 DPM_F_BLEND or DPM_F_NOISE (a record that sets the flag and one of the two other guidance flags
                                 is reported by this flag's checks); DPM_FORM_UNIPC; a double state; eps_stride other than 0 or
                                 P; device-resident coefficients.  No output byte is written in any error case.  One workgroup
                                 per sample (stage_zstar_kernel); such a stage runs on its own in a multi-request launch, in
                                 every mode of dpm_stage_launch_multi */

#define DPM_F_CFG2_PERP 8192u /* version 220, with guidance == DPM_GUIDE_CFG2 only (else DPM_ERR_ARG); never set by the planner.
                                 (The table_mode bit 8192 is a different space and stays unassigned.)
                                 Perp-Neg (Armandpour et al. 2023, "Re-imagine the Negative Prompt Algorithm"): the negative
                                 condition's direction is taken perpendicular to the positive one's, per sample, before it is
                                 subtracted.  Operands as under DPM_GUIDE_CFG2: e0 = the raw output under the positive
                                 condition, e1 = the unconditional raw output, g = the raw output under the negative condition.
                                 Scalars: s = dpm_stage.cfg_scale (guidance scale), w = dpm_stage.cg_scale (negative scale; the
                                 planner writes 0 there, the caller overwrites it).  For each sample of the launch, with
                                 P = n / batch elements, on the RAW outputs widened to fp32 (as under DPM_F_CFG_ZSTAR):
                                   d0   = o_c - o_u ;  d2 = o_n - o_u       fp32, one rounding each
                                   S_nd = sum (double)d2 * (double)d0       products exact in double; sums in double, any order
                                   S_dd = sum (double)d0 * (double)d0
                                   a    = S_dd > 0 ? (float)(S_nd / S_dd) : 0.f     one double division, one rounding; a zero or
                                                                            NaN S_dd gives a = 0: defined behaviour
                                   perp = d2 - a * d0                       fp32, one rounding per operation, no fused multiply-add
                                   gd   = o_u + s * (d0 - w * perp)         likewise
                                   eps  = noise prediction of the raw output gd (x_start / v / score conversion on xe), then
                                          DPM_F_TO_X0, the update form (LIN1 .. DENOISE, DPM_F_BASE_HIST included),
                                          DPM_F_STORE_M and the stores, all fp32
                                 Nothing after the loads is rounded to the network's dtype, and the model values are never half
                                 tensors under the flag.  Three identities follow from the arithmetic:
                                   g == e0 (negative = positive): d2 = d0, a = 1, perp = 0 and gd = o_u + s * d0;
                                   g == e1: d2 = 0, a = 0, perp = 0 and the same gd;
                                   e0 == e1: d0 = 0, a = 0 and gd = o_u - s * (w * d2).
                                 DPM_ERR_ARG: the flag without DPM_GUIDE_CFG2; s or w not finite; e1 or g NULL; an unknown form.
                                 DPM_ERR_UNSUPPORTED (this version): everything DPM_GUIDE_CFG2 refuses -- DPM_F_THRESH,
                                 DPM_F_BLEND, DPM_F_NOISE, DPM_F_USER_X0, DPM_FORM_UNIPC, a non-NULL x_out2, a double state,
                                 eps_stride other than 0 or P, device-resident coefficients --; a batch above 2^31 - 1; a
                                 table-mode call without DPM_TABLE_PERP (version 221; DPM_TABLE_PAIR rows have no per-sample
                                 pass) that carries the flag.  A record
                                 that sets one of DPM_F_CFG_RESCALE / _APG / _ZSTAR is reported by those flags' checks first,
                                 and every check of DPM_GUIDE_CFG2 speaks before this flag's own.  No output byte is written in
                                 any error case.  One workgroup per sample (stage_perp_kernel); such a stage runs on its own in
                                 a multi-request launch, in every mode of dpm_stage_launch_multi */

/* buffer roles for the host-side loop */
enum { DPM_SRC_STATE = 0, DPM_SRC_TMP = 1 };

/* ---- one stage = one network evaluation + one fused kernel ----------------------------- */
typedef struct dpm_stage {
  int32_t index;       /* position in the plan                                                   */
  int32_t form;        /* DPM_FORM_*                                                             */
  uint32_t flags;      /* DPM_F_*                                                                */
  int32_t model_type;  /* DPM_MODEL_*  : conversion applied to the raw network output            */
  int32_t guidance;    /* DPM_GUIDE_*                                                            */
  int32_t outer_step;  /* `step` handed to correcting_xt_fn(x, t, step) for this stage's output  */
  int32_t emits_state; /* 1: x_out is a solver state x_i (goes to `intermediates`), 0: mid-stage */
  int32_t x_src;       /* DPM_SRC_*: which buffer is the update's x                              */
  int32_t xe_src;      /* DPM_SRC_*: which buffer the network was evaluated on                   */
  int32_t h1_slot;     /* history slot read as h1, -1 = none                                     */
  int32_t h2_slot;     /* history slot read as h2, -1 = none                                     */
  int32_t m_slot;      /* history slot written with mn, -1 = none                                */
  float t_eval;        /* continuous time of the network evaluation (fp32 as the reference)      */
  float t_input;       /* model time label: (t - 1/N)*1000 for discrete schedules (ref :278)     */
  float t_out;         /* continuous time of x_out                                               */
  float alpha_e;       /* alpha(t_eval)                                                          */
  float sigma_e;       /* sigma(t_eval)                                                          */
  float cfg_scale;     /* guidance_scale as fp32 (ref :330)                                      */
  float cg_scale;      /* fl(guidance_scale * sigma(t_eval))  (ref :321); DPM_F_CFG_RESCALE: phi; DPM_F_CFG_APG: eta;
                          DPM_GUIDE_CFG2: s2, the scale of the second condition (the planner writes 0); with
                          DPM_F_CFG2_PERP: w, the negative scale                                                   */
  float cx, c0, c1, c2; /* update coefficients, reference association (see kernels)              */
  float k[5];          /* difference-quotient scalars: 1/r0, 1/r1, ...                           */
  float thr_ratio;     /* dynamic_thresholding_ratio;  DPM_F_CFG_APG: the norm threshold r       */
  float thr_max;       /* thresholding_max_val;        DPM_F_CFG_APG: the momentum beta          */
  float blend_alpha;  /* DPM_F_BLEND: alpha at the time the known image is noised to (add_noise, ref :1028)  */
  float blend_sigma;   /* DPM_F_BLEND: sigma at that time                                        */
} dpm_stage;

/* The float fields of dpm_stage in double: a double-precision run (state DPM_DTYPE_F64; dpm_plan_desc.precision = 1).
   The reference computes in whatever dtype torch's type promotion yields (ref :14, :105-107, :573-576): with a double state
   and NoiseScheduleVP(dtype=torch.float64) every scalar of a step is a double.  dpm_plan_stage_f64 returns these next to
   the dpm_stage of the same index (whose float fields are the doubles rounded); a launch finds them through
   dpm_buffers.coef64 (NULL: the launch converts the dpm_stage's floats exactly -- a double state on an fp32 schedule, where
   the reference's scalars ARE fp32 tensors). */
typedef struct dpm_stage_f64 {
  double t_eval, t_input, t_out, alpha_e, sigma_e, cfg_scale, cg_scale, cx, c0, c1, c2, k[5], thr_ratio, thr_max, blend_alpha,
      blend_sigma;
  int32_t time_f64;  /* dtype of the reference's time TENSORS in this run: bit 0 set = the tensor the network is called with
                        at t_eval is a double (singlestep inner nodes, logSNR grids: they come out of inverse_lambda on double
                        tables), clear = an fp32 tensor (torch.linspace grids, ref :472-477) and t_input was computed in fp32
                        (ref :278); bit 1: the same for t_out (the time handed to correcting_xt_fn)                       */
  int32_t reserved;
} dpm_stage_f64;

/* ---- per-call options (optional; NULL or all-zero = the defaults) ------------------------ */
typedef struct dpm_launch_opts {
  int32_t cluster_in_graph; /* 1: dynamic thresholding keeps its workgroup clusters under stream capture also for samples
                               that fit one workgroup (default 0: one workgroup per sample there -- a replayed graph runs
                               outside the library's per-device chain of clustered launches)                          */
  int32_t no_fuse;          /* 1: dpm_stage_launch_multi / dpm_plan_run_multi launch request by request (results are
                               identical; what a single request's stage costs next to the fused launch)               */
  int32_t thr_spin_limit;   /* > 0: polls (a microsecond or two each) before a wait on a cluster peer gives up and the
                               workgroup finishes its sample alone; 0 = the default, 4096                             */
  int32_t per_request_stages; /* 1: dpm_stage_launch_multi reads `st` as an array of n_req stage records, request r is
                               advanced by st[r] (version 202; see there)                                             */
  uint32_t noise_seed_lo;   /* version 203: the 64-bit seed of DPM_F_NOISE stages (Philox key), low and high word (were */
  uint32_t noise_seed_hi;   /* reserved[0..1]).  dpm_stage_launch_multi fuses noise stages like the others (version 204) */
                            /* and still keys request r's generator with the seed of its own bs[r].opts (NULL: seed 0); */
                            /* dpm_plan_run_multi hands request r its rbs[r].opts there; dpm_graph_create bakes the     */
                            /* seed of rb->opts into the graph                                                          */
  int32_t fuse_shapes;      /* version 207 (was reserved[0]); read from bs[0].opts, together with per_request_stages == 1
                               only.  1: the requests of a fused group need not agree on n and batch (see
                               dpm_stage_launch_multi); 0: every call groups and launches as before version 207          */
  int32_t table_mode;       /* version 208 (was reserved[0]); read from bs[0].opts, together with per_request_stages == 1
                               only.  0: every call as before version 208; DPM_TABLE_FILL / DPM_TABLE_LAUNCH: see "Table
                               mode" at dpm_stage_launch_multi                                                            */
} dpm_launch_opts;
enum { DPM_TABLE_FILL = 1, DPM_TABLE_LAUNCH = 2 };
enum { DPM_TABLE_NOISE = 4 }; /* version 209: a flag OR-ed onto DPM_TABLE_FILL / DPM_TABLE_LAUNCH (table_mode 5 / 6): SDE stages
                                 take rows too, each with a noise record behind the rows */
enum { DPM_TABLE_THRESH = 8 }; /* version 210: a flag OR-ed onto DPM_TABLE_FILL / DPM_TABLE_LAUNCH, with or without DPM_TABLE_NOISE
                                  (table_mode 9 / 10 / 13 / 14): thresholded stages of small samples take rows too */
enum { DPM_TABLE_BLEND = 32 }; /* version 211: a flag OR-ed onto DPM_TABLE_FILL / DPM_TABLE_LAUNCH, with or without the two flags
                                   above: DPM_F_BLEND stages take rows too, each with a blend record behind the rows.  (Bit 16
                                   is unassigned: table_mode 16 .. 31 stay DPM_ERR_ARG, as in version 210.) */
enum { DPM_TABLE_RESCALE = 128 }; /* version 213: a flag OR-ed onto DPM_TABLE_FILL / DPM_TABLE_LAUNCH, with or without the three
                                     flags above: DPM_F_CFG_RESCALE stages take rows too, rows like any other.  (Bits 16 and 64
                                     are unassigned: table_mode 16 .. 31 and 64 .. 127 stay DPM_ERR_ARG.) */
enum { DPM_TABLE_APG = 512 }; /* version 215: a flag OR-ed onto DPM_TABLE_FILL / DPM_TABLE_LAUNCH, with or without the four flags
                                 above: DPM_F_CFG_APG stages take rows too, each with an APG record behind the rows, and the
                                 running average of every DPM_F_CFG_APG request of the call is its dpm_buffers.thr_hint.  (Bits
                                 16, 64 and 256 are unassigned: table_mode 16 .. 31, 64 .. 127 and 256 .. 511 stay DPM_ERR_ARG,
                                 and so does every mode from 512 on that has one of those bits.) */
enum { DPM_TABLE_ZSTAR = 4096 }; /* version 217: a flag OR-ed onto DPM_TABLE_FILL / DPM_TABLE_LAUNCH, with or without the five
                                    flags above: DPM_F_CFG_ZSTAR stages take rows too, rows like any other, no records.  (4096 is
                                    the lowest free bit: 16, 64, 256 and 1024 are unassigned, and so is 2048 -- table_mode 2048 |
                                    513 is pinned as DPM_ERR_ARG since version 215.  Every mode with one of the bits 16, 64, 256,
                                    1024, 2048, or a bit from 8192 on, stays DPM_ERR_ARG.) */
enum { DPM_TABLE_PAIR = 16384 }; /* version 219: a flag OR-ed onto DPM_TABLE_FILL / DPM_TABLE_LAUNCH, with or without the six
                                    flags above: DPM_GUIDE_CFG2 stages take rows too, each with a pair record behind the rows,
                                    and a DPM_GUIDE_CFG2 request of the call may carry x_out2 together with a third copy of x_out
                                    in its dpm_buffers.thr_hint.  (Bit 8192 is unassigned -- table_mode 8192 | 1 is pinned as
                                    DPM_ERR_ARG since version 217.  Every mode with one of the bits 16, 64, 256, 1024, 2048,
                                    8192, or a bit from 32768 on, stays DPM_ERR_ARG.) */
enum { DPM_TABLE_PERP = 65536 }; /* version 221: a flag OR-ed onto DPM_TABLE_FILL / DPM_TABLE_LAUNCH, with or without the seven
                                    flags above: DPM_F_CFG2_PERP stages take rows too, each with a pair record (DPM_TABLE_PAIR_BYTES,
                                    in the pair-record section, which is present under either flag), and a flagged DPM_GUIDE_CFG2
                                    request of the call may carry x_out2 together with a third copy of x_out in its
                                    dpm_buffers.thr_hint.  (Bit 32768 is unassigned -- table_mode 32768 | 1 is pinned as
                                    DPM_ERR_ARG since version 219.  Every mode with one of the bits 16, 64, 256, 1024, 2048,
                                    8192, 32768, or a bit from 131072 on, stays DPM_ERR_ARG.) */
#define DPM_TABLE_MAGIC 0x4c425444u /* "DTBL", the first word of a table's header */
#define DPM_TABLE_NOISE_BYTES 32    /* one noise record (= dpm_sizeof(DPM_SIZEOF_TABLE_NOISE)) */
#define DPM_TABLE_BLEND_BYTES 48    /* one blend record (= dpm_sizeof(DPM_SIZEOF_TABLE_BLEND)) */
#define DPM_TABLE_APG_BYTES 32      /* one APG record (= dpm_sizeof(DPM_SIZEOF_TABLE_APG)) */
#define DPM_TABLE_PAIR_BYTES 16     /* one pair record (= dpm_sizeof(DPM_SIZEOF_TABLE_PAIR)); a Perp-Neg row's record too */

/* ---- buffers of one launch ------------------------------------------------------------- */
typedef struct dpm_buffers {
  const void* x;    /* state the update starts from                          [n] state dtype     */
  const void* xe;   /* state the network saw (NULL = same as x)              [n] state dtype     */
  const void* e0;   /* raw network output (conditional half under CFG)       [n] eps dtype       */
  const void* e1;   /* raw unconditional output (CFG only)                   [n] eps dtype       */
  const void* g;    /* classifier gradient (classifier guidance); DPM_GUIDE_CFG2: the raw
                       output under the second condition                   [n] eps dtype       */
  const void* h1;   /* cached model value                                    [n] state dtype     */
  const void* h2;   /* cached model value                                    [n] state dtype     */
  void* x_out;      /* result of the update                                  [n] state dtype     */
  void* m_out;      /* new model value (only if DPM_F_STORE_M)               [n] state dtype     */
  void* workspace;  /* thresholding scratch, dpm_threshold_workspace_bytes() bytes (may be NULL);
                       DPM_F_CFG_APG with a momentum: the running average, n fp32 values -- outside a
                       DPM_TABLE_APG call, where thr_hint holds it                                   */
  int64_t n;          /* total elements = batch * per_sample                                     */
  int64_t batch;      /* number of independent samples                                           */
  int32_t state_dtype; /* DPM_DTYPE_* of x, xe, h1, h2, x_out, m_out                             */
  int32_t eps_dtype;   /* DPM_DTYPE_* of e0, e1, g                                               */
  /* ---- optional extensions (zero / NULL = off) ---- */
  void* x_out2;        /* second copy of x_out: the other half of the [2B,...] network input under
                          classifier-free guidance (replaces torch.cat([x]*2), ref :326)   [n] state dtype;
                          with DPM_F_STORE_XC: the corrected state of a DPM_FORM_UNIPC stage instead       */
  int64_t eps_stride;  /* elements between consecutive samples of e0 / e1 (0 = contiguous): the network output
                          is a channel slice out[:, :C] of a learned-variance model's [B,2C,H,W] output
                          (runners/diffusion.py:596-603); a sample's C*H*W elements stay contiguous      */
  const void* mask;    /* DPM_F_BLEND: mask, state dtype, mask_period elements, indexed i % mask_period  */
  const void* blend_a; /* DPM_F_BLEND: known image (or, with blend_b NULL, the state to blend in)  [n]   */
  const void* blend_b; /* DPM_F_BLEND: noise [n], NULL = blend_a is used as is                          */
  int64_t mask_period; /* n for a full mask, H*W for a [H,W] mask, C*H*W for a [1,C,H,W] mask           */
  int32_t inputs_resident; /* cache-policy hint.  0 (default): a network ran since x / the cached values were
                          written, the streams come from HBM -> streaming loads.  1: the immediately preceding launch
                          wrote them (frozen-model loops; dpm_plan_run sets it when there is no model callback) ->
                          default cache policy, they are expected in the 256 MiB Infinity Cache                  */
  int32_t noise_sample0; /* version 209 (was `reserved`).  The buffers are samples [noise_sample0, noise_sample0 + batch) of the
                          tensor the noise contract indexes: element i of the buffers takes the z of element
                          noise_sample0 * (n / batch) + i.  Honoured by the rows of a DPM_TABLE_NOISE call's SDE stages only;
                          non-zero anywhere else -- table_mode 0 / 1 / 2, a stage without DPM_F_NOISE, a request that fits no
                          fused group --, negative, or with noise_sample0 * (n / batch) not a multiple of 4: DPM_ERR_ARG */
  float* thr_hint;     /* DPM_F_THRESH, optional (NULL = off): DPM_THR_HINT_WORDS floats per sample that persist from stage
                          to stage of ONE trajectory -- the kernel's private state (content undefined to the caller; no
                          initialisation needed: the stage with index 0 resets it).  [0], [1]: the selected order statistic
                          of |x0| in the previous two thresholded stages, from which a clustered launch predicts this
                          stage's select bound (a correct prediction saves the bound search and shrinks the exchange; a
                          wrong one is detected and costs one extra exchange, never exactness); [2]: route taken
                          (diagnostics: 1 predicted, 2 prediction rejected, 3 single exchange, 4 general); [3]: entries of
                          the last union gathered (diagnostics).
                          DPM_F_CFG_APG with a momentum in a call that carries DPM_TABLE_APG (version 215; the flag excludes
                          DPM_F_THRESH, so no APG stage reads a hint): the RUNNING AVERAGE, n fp32 values in the state's flat
                          order, read and written in place -- private state that persists over one trajectory, as the hint
                          is; the caller zero-fills it where a trajectory starts.  NULL with beta != 0: DPM_ERR_ARG.
                          DPM_GUIDE_CFG2 in a call that carries DPM_TABLE_PAIR (version 219; the guidance excludes DPM_F_THRESH,
                          so no such stage reads a hint): the THIRD copy of x_out, n values of the STATE dtype, written where
                          x_out2 is -- both NULL or both set, else DPM_ERR_ARG                                            */
  const dpm_launch_opts* opts; /* per-call options, NULL = defaults (version 200; dpm_stage_launch_multi reads bs[0].opts) */
  const dpm_stage_f64* coef64; /* DPM_DTYPE_F64 launches: the stage's scalars in double (NULL: the dpm_stage's floats, exactly) */
} dpm_buffers;

/* ---- noise schedule (NoiseScheduleVP, ref :6-167) --------------------------------------- */
typedef struct dpm_schedule dpm_schedule;

/* discrete-time schedules; `clip` != 0 applies numerical_clip_alpha at lambda = -5.1 (ref :114-125). */
DPM_API int dpm_schedule_create_betas_f32(const float* betas, int n, int clip, dpm_schedule** out);           /* ref :100 */
DPM_API int dpm_schedule_create_betas_f64(const double* betas, int n, int clip, dpm_schedule** out);
DPM_API int dpm_schedule_create_alphas_cumprod_f32(const float* ac, int n, int clip, dpm_schedule** out);      /* ref :103 */
DPM_API int dpm_schedule_create_alphas_cumprod_f64(const double* ac, int n, int clip, dpm_schedule** out);
DPM_API int dpm_schedule_create_log_alpha(const float* log_alpha, int n, dpm_schedule** out);                  /* ready table */
/* numerical_clip_alpha on its own (ref :114-125): *out_len = number of leading entries of `log_alphas` whose
   half-logSNR is >= clipped_lambda (the reference returns log_alphas[:out_len]); arithmetic in the array's type */
DPM_API int dpm_numerical_clip_len_f32(const float* log_alphas, int n, double clipped_lambda, int* out_len);
DPM_API int dpm_numerical_clip_len_f64(const double* log_alphas, int n, double clipped_lambda, int* out_len);
DPM_API int dpm_schedule_create_linear(double beta_0, double beta_1, dpm_schedule** out);                      /* ref :109-112 */
/* the continuous-time 'cosine' schedule of the older vendored revision (examples/score_sde_pytorch/dpm_solver.py
   :114-124,:134-137,:171-175): s = 0.008, T = 0.9946 (the caller's default end time) */
DPM_API int dpm_schedule_create_cosine(dpm_schedule** out);
/* NoiseScheduleVP(dtype=torch.float64) (ref :14, :105-107): the tables keep the double values they were computed in (the
   *_f64 constructors) instead of their fp32 roundings -- what double-precision plans and dpm_schedule_eval_f64 read.  Part of
   construction: call it right after dpm_schedule_create_*, before the handle is shared. */
DPM_API int dpm_schedule_set_table_dtype(dpm_schedule* s, int dtype /* DPM_DTYPE_F32 | DPM_DTYPE_F64 */);
DPM_API int dpm_schedule_tables_f64(const dpm_schedule* s, const double** log_alpha, const double** t_array, int* K);
DPM_API void dpm_schedule_destroy(dpm_schedule* s);
DPM_API int dpm_schedule_is_discrete(const dpm_schedule* s);
DPM_API int dpm_schedule_total_N(const dpm_schedule* s);                                                       /* ref :106,:110 */
/* borrowed pointers into the handle: log_alpha_array / t_array of ref :105,:107 (K floats each). */
DPM_API int dpm_schedule_tables(const dpm_schedule* s, const float** log_alpha, const float** t_array, int* K);
/* marginal_log_mean_coeff / marginal_alpha / marginal_std / marginal_lambda / inverse_lambda (ref :127-167) */
DPM_API int dpm_schedule_eval(const dpm_schedule* s, int what, const float* in, int n, float* out);
DPM_API int dpm_schedule_eval_f64(const dpm_schedule* s, int what, const double* in, int n, double* out);  /* double times / tables */

/* ---- time grids (ref :453-539) ---------------------------------------------------------- */
DPM_API int dpm_time_steps(const dpm_schedule* s, int skip_type, double t_T, double t_0, int N, float* out /* N+1 */);
DPM_API int dpm_singlestep_orders(int steps, int order, int* orders /* >= steps */, int* n_orders);
DPM_API int dpm_singlestep_grid(const dpm_schedule* s, int steps, int order, int skip_type, double t_T, double t_0,
                        float* outer /* >= steps+1 */, int* orders /* >= steps */, int* n_orders);

/* ---- plan: DPM_Solver.sample() unrolled into stages (ref :1047-1245) ---------------------- */
typedef struct dpm_plan_desc {
  int32_t algorithm_type;    /* DPM_ALGO_*                        */
  int32_t method;            /* DPM_METHOD_*                      */
  int32_t order;             /* 1..3                              */
  int32_t steps;             /* NFE                               */
  int32_t skip_type;         /* DPM_SKIP_*                        */
  int32_t solver_type;       /* DPM_SOLVER_* (DPM_ALGO_UNIPC: _UNIPC_BH1 / _UNIPC_BH2) */
  int32_t lower_order_final; /* bool                              */
  int32_t denoise_to_zero;   /* bool                              */
  int32_t model_type;        /* DPM_MODEL_*                       */
  int32_t guidance;          /* DPM_GUIDE_*                       */
  int32_t thresholding;      /* bool: correcting_x0_fn == "dynamic_thresholding" */
  int32_t precision;         /* 0: scalars in fp32, the reference's default (fp32 schedule tables and times); 1: in double --
                                a double state on a schedule declared dtype=float64 (dpm_schedule_set_table_dtype), or whose
                                times are doubles: dpm_plan_stage_f64 then returns the doubles (version 200; was `reserved`) */
  double t_start;            /* t_T                               */
  double t_end;              /* t_0                               */
  double guidance_scale;
  double thr_ratio;          /* dynamic_thresholding_ratio        */
  double thr_max;            /* thresholding_max_val              */
} dpm_plan_desc;

typedef struct dpm_plan dpm_plan;
DPM_API int dpm_plan_create(const dpm_schedule* s, const dpm_plan_desc* d, dpm_plan** out);
DPM_API void dpm_plan_destroy(dpm_plan* p);
DPM_API int dpm_plan_num_stages(const dpm_plan* p);
DPM_API int dpm_plan_num_slots(const dpm_plan* p);                 /* history buffers the loop needs      */
DPM_API int dpm_plan_stage(const dpm_plan* p, int i, dpm_stage* out);
DPM_API int dpm_plan_stage_f64(const dpm_plan* p, int i, dpm_stage_f64* out);   /* double-precision plans only */
DPM_API int dpm_plan_timesteps(const dpm_plan* p, float* out, int cap, int* n); /* solver grid t_0..t_K    */

/* ---- coefficient builders for the reference's public per-update methods -------------------- */
/* dpm_solver_first_update (ref :547-592) */
DPM_API int dpm_coef_first(const dpm_schedule* s, int algo, float t_s, float t_t, dpm_stage* out);
/* multistep_dpm_solver_update (ref :932-954): t_prev[0..order-1] oldest..newest */
DPM_API int dpm_coef_multistep(const dpm_schedule* s, int algo, int solver_type, int order, const float* t_prev, float t_t,
                       dpm_stage* out);
/* singlestep_dpm_solver_update (ref :906-930): fills `order` stages.  r_mode 0: r1/r2 are the reference's
   Python-float defaults or user floats (double arithmetic then one fp32 rounding), 1: fp32 tensors. */
DPM_API int dpm_coef_singlestep(const dpm_schedule* s, int algo, int solver_type, int order, float t_s, float t_t,
                        double r1, double r2, int r_mode, dpm_stage* out /* [order] */);
/* fill the prologue scalars (alpha_e, sigma_e, t_input, guidance) of a stage evaluated at t */
DPM_API int dpm_coef_prologue(const dpm_schedule* s, float t_eval, int model_type, int guidance, double guidance_scale,
                      dpm_stage* inout);

/* the same in double (a double-precision evaluation: double time tensors, or a schedule declared dtype=float64): out = the
   integer fields + the doubles rounded, out64 = the doubles.  time_f64: the caller's time tensors are doubles (else fp32
   tensors whose values arrive converted exactly) -- decides the dtype the model time label is computed in (ref :278).
   dpm_coef_first is dpm_coef_multistep_f64 with order 1. */
DPM_API int dpm_coef_multistep_f64(const dpm_schedule* s, int algo, int solver_type, int order, const double* t_prev, double t_t,
                           int time_f64, dpm_stage* out, dpm_stage_f64* out64);
DPM_API int dpm_coef_singlestep_f64(const dpm_schedule* s, int algo, int solver_type, int order, double t_s, double t_t, int time_f64,
                            double r1, double r2, int r_mode, dpm_stage* out /* [order] */, dpm_stage_f64* out64 /* [order] */);
DPM_API int dpm_coef_prologue_f64(const dpm_schedule* s, double t_eval, int time_f64, int model_type, int guidance, double guidance_scale,
                          dpm_stage* inout, dpm_stage_f64* inout64);

/* ---- device side --------------------------------------------------------------------------- */
/* one fused stage kernel, asynchronous on `stream` */
DPM_API int dpm_stage_launch(const dpm_stage* st, const dpm_buffers* b, void* stream);
/* The same stage of n_req independent requests (same plan position: one dpm_stage; same n, batch and dtypes; each its
   own buffers) as ONE fused launch per group of DPM_MULTI_MAX requests: a server that keeps R sampling requests in
   flight pays a launch's ramp-up and drain once per R x (5 n s) bytes instead of once per 5 n s -- with inputs coming
   from HBM (a network ran in between) that is 8.5 -> ~6.7 us per [256,4,64,64] fp16 request-stage.  Stages with
   dynamic thresholding become one thresholding launch over all requests' samples (a batch of n_req * batch: smaller
   clusters or none -- 32 requests of [32,3,64,64] cost about what one [1024,3,64,64] does), provided clustered shapes
   find a DIFFERENT workspace in every request; classifier-free guidance keeps its duplicate store (x_out2).  SDE stages
   (DPM_F_NOISE, version 204) are fused as well: the stage index and the scale are the launch's, the seed is each request's
   own -- bs[r].opts->noise_seed_lo / _hi, 0 where bs[r].opts is NULL -- and every request gets the bits of its single
   launch (the noise contract: z depends on seed, stage index and element index only).  Stages
   neither family covers (mask blend, classifier guidance, strided or
   unaligned buffers, the singlestep mid-stages, thresholding with a shared workspace) are launched request by
   request; results are identical either way.
   Per-request stages (version 202): with bs[0].opts->per_request_stages == 1, `st` points at n_req stage records and
   request r is advanced by st[r] -- requests that arrived at different times, at different positions of plans with
   different step counts or orders (continuous batching).  Every request is checked as dpm_stage_launch checks it (same
   error texts; nothing is launched when one fails).  Requests whose stage is first-order, 2M-style second-order (TWO),
   multistep third-order (MS3) or -- version 206 -- UniPC (DPM_FORM_UNIPC without DPM_F_STORE_XC, whatever its DPM_F_UNIPC_DP /
   _P2 bits), without thresholding, mask blend or classifier guidance, whose evaluation state is the
   state and whose buffers are dense and 16-byte aligned, are fused -- 16 per launch: the records travel in the kernel's
   arguments, within HIP's 4 KiB -- with every other
   request that agrees with them on dtypes, n, batch, model type, guidance kind, DPM_F_TO_X0 and DPM_F_NOISE (SDE stages
   -- LIN1 / TWO -- form groups of their own, each request with its own stage index, scale and seed); the rest are launched
   one by one.  Groups fill in call order (first come, first grouped).  MS3 and UNIPC stages never share a group: the first
   of the two forms to join a group decides which it takes, stages of the other form open a later group; first- and
   second-order stages join either, so a pool of UniPC requests -- first-order at stage 0, UNIPC afterwards -- and 2M
   requests is one launch per 16 requests. Results are identical either way; dpm_launch_opts.no_fuse launches every request on its own.
   Mixed shapes (version 207): with bs[0].opts->fuse_shapes == 1 as well, a group's requests need not agree on n and batch --
   every other rule above stays (dtypes, model type, guidance kind, DPM_F_TO_X0, DPM_F_NOISE, dense 16-byte aligned buffers of
   whole 8-element groups, call order, 16 per launch, MS3 apart from UNIPC).  A group whose members share one n is launched
   exactly as without the flag; a group with at least two different n is ONE launch whose tile space is the members' tiles
   back to back, each request advanced over its own n with the bits of its single launch.  (A group of 2^31 or more
   super-tiles of 2048 or 4096 elements is launched member by member.)
   Table mode (version 208): the 16 requests per launch above are what HIP's 4 KiB of kernel arguments hold.  With
   bs[0].opts->table_mode != 0 (and per_request_stages == 1, fuse_shapes == 0) the records of a group of MORE than 16 requests
   travel as rows of a table in device memory, and the group -- whatever its size, below 2^31 super-tiles -- is ONE launch
   (stage_kernel_table / stage_kernel_table_unipc).  The table lives in bs[0].workspace: at least
   dpm_sizeof(DPM_SIZEOF_TABLE_HEADER) + n_req * dpm_sizeof(DPM_SIZEOF_TABLE_ROW) bytes, 16-byte aligned (NULL or misaligned:
   DPM_ERR_ARG; so is DPM_F_THRESH in st[0], whose workspace would mean two things -- thresholded requests at r > 0 keep
   theirs).  Two calls with the SAME st / bs arrays make a tick:
     DPM_TABLE_FILL    bs[0].workspace is HOST memory.  Checks every request as mode 0 does (same error texts, nothing written
                       when one fails), groups them by the rules above without the cap of 16, and writes
                         header  4 x uint32: DPM_TABLE_MAGIC, dpm_version(), n_req, the number of groups with rows
                         rows    from byte dpm_sizeof(DPM_SIZEOF_TABLE_HEADER) on, dpm_sizeof(DPM_SIZEOF_TABLE_ROW) bytes
                                 each: for every group of more than 16 members a run of consecutive rows, members in call
                                 order, the runs in the order their groups open.  A row is 8 pointers -- x, e0, e1, h1, h2,
                                 x_out, m_out, x_out2 of the request's dpm_buffers -- followed by 20 32-bit words of stage
                                 scalars in the kernels' own layout (opaque: made by the library, read by the library).
                       Groups of 2..16 members write no rows.  Launches nothing and makes no HIP call at all: it runs on a
                       machine without a GPU.
     DPM_TABLE_LAUNCH  bs[0].workspace is DEVICE memory holding a byte copy of what DPM_TABLE_FILL wrote; the copy is the
                       CALLER's (one hipMemcpyAsync on `stream` between the two calls), and a stale copy is the caller's
                       error like any stale pointer in dpm_buffers.  Repeats checks and grouping on the host (the same
                       function: the same row order); a group with rows is ONE launch over its run of rows, every other
                       group and every request that fits no group goes exactly as in mode 0.  The library copies nothing,
                       allocates nothing and synchronises nothing.
   SDE stages (without DPM_TABLE_NOISE), mixed n (fuse_shapes), thresholding (without DPM_TABLE_THRESH), mask blend (without
   DPM_TABLE_BLEND), classifier guidance, DPM_F_STORE_XC, DPM_F_CFG_RESCALE (without DPM_TABLE_RESCALE), DPM_F_CFG_APG (without DPM_TABLE_APG), DPM_F_CFG_ZSTAR (without DPM_TABLE_ZSTAR) and DPM_GUIDE_CFG2 (without DPM_TABLE_PAIR) are outside the table kernels: in a table call such requests take exactly the path they take in mode 0.
   Every request gets the bits of its own dpm_stage_launch.
   SDE rows (version 209): DPM_TABLE_FILL | DPM_TABLE_NOISE and DPM_TABLE_LAUNCH | DPM_TABLE_NOISE (table_mode 5 / 6) make the
   same tick with SDE stages in the table (stage_kernel_table_noise).  EVERY fusable DPM_F_NOISE request -- the rules above,
   LIN1 / TWO -- then owns a row, whatever the size of its group, down to a group of one; the groups are those of mode 0
   without the cap of 16, one run of rows and one launch each.  ODE and UniPC groups keep the rules above (rows from 17
   members).  Behind the rows the table holds one noise record per row: the record of table row i (counted over all runs) is
   the DPM_TABLE_NOISE_BYTES bytes at dpm_sizeof(DPM_SIZEOF_TABLE_HEADER) + n_req * dpm_sizeof(DPM_SIZEOF_TABLE_ROW) +
   DPM_TABLE_NOISE_BYTES * i, n_req the call's; the table is dpm_sizeof(DPM_SIZEOF_TABLE_HEADER) + n_req *
   (dpm_sizeof(DPM_SIZEOF_TABLE_ROW) + DPM_TABLE_NOISE_BYTES) bytes.  A record is 8 x uint32: seed lo, seed hi (the request's
   own bs[r].opts, NULL: 0), st[r].index, the bits of st[r].c2, g0 lo, g0 hi, 0, 0.  g0 = bs[r].noise_sample0 * (n / batch) / 4
   is added to the index of every Philox block of the row (64-bit), so the row's element i takes the z of element
   noise_sample0 * (n / batch) + i of the noise contract: with noise_sample0 = k, a row that holds sample k of a larger
   request gets the bits that sample has in the request's own launch; 0 gives the bits of the row's own dpm_stage_launch.
   FILL writes the records of SDE rows only and leaves every other byte of the record section untouched.  Without the flag
   (table_mode 1 / 2) SDE requests take their mode-0 path and write no rows, as in version 208.
   Thresholded rows (version 210): DPM_TABLE_THRESH OR-ed onto either mode, alone or with DPM_TABLE_NOISE (table_mode 9 / 10,
   13 / 14), makes the same tick with thresholded stages in the table (stage_thresh_kernel_table: one workgroup of 512 threads
   per sample, the sample's x0 in its LDS, no cluster, no workspace, no wait on another workgroup).  A DPM_F_THRESH request
   owns a row when it passes every rule of the fused groups above apart from the DPM_F_THRESH bit -- form LIN1 / TWO / MS3, or
   DPM_FORM_DENOISE (the thresholded last stage of denoise_to_zero, its buffers checked as LIN1's), guidance none or CFG,
   evaluation state = state, dense buffers of whole 8-element groups, 16-byte aligned, x_out2 only under CFG, a 2- or 4-byte
   dtype pair --, has neither DPM_F_BLEND nor DPM_F_NOISE, and its SAMPLE, n / batch elements, is a multiple of 4 and
   at most 12288 (the kernel works per sample, in 4-element accesses, and a sample has to fit one workgroup's LDS; n being a
   multiple of 8 is not enough: 4 samples of 10 elements own no row).  Such requests form groups of their own -- never with an un-thresholded request -- that agree on
   dtypes, n, batch, model type, guidance kind, DPM_F_TO_X0 and on the bit patterns of thr_ratio and thr_max; the forms
   share a group.  Every group, from ONE member on, is one run of rows and ONE launch (below 2^31 samples), the runs in the
   order the groups open, among those of the other families.  A thresholded row is a row like any other -- the 8 pointers and
   the 20 words of stage scalars, which already say which prologue the stage takes; rows of other requests, the row size and
   the record section are byte for byte those of version 209, and there is no further section (dpm_sizeof(11), like
   dpm_sizeof(9), is 0).  Such a request reads no dpm_buffers.workspace and no thr_hint, so st[0] may be one: bs[0].workspace
   is the table.  A thresholded request that does not qualify (a larger sample, a mask blend, unaligned buffers ...) takes its
   mode-0 path in the same call, with the workspace that path needs; as st[0] it is DPM_ERR_ARG as before.  Without the flag
   every call is version 209's, the refusal of DPM_F_THRESH in st[0] included.  FILL still makes no HIP call; LAUNCH copies,
   allocates and synchronises nothing.  Every sample gets the bits of its request's own dpm_stage_launch.
   Blend rows (version 211): DPM_TABLE_BLEND OR-ed onto either mode, alone or with DPM_TABLE_NOISE / DPM_TABLE_THRESH, makes the
   same tick with mask-blend stages (DPM_F_BLEND: inpainting, DiffEdit) in the table (stage_kernel_table_blend: stage_kernel_table
   over the forms LIN1 / TWO / MS3 with the blend epilogue of dpm_stage_launch).  A DPM_F_BLEND request owns a row when it
   passes every rule of the fused groups above apart from the DPM_F_BLEND bit -- guidance none or CFG, evaluation state =
   state, dense buffers of whole 8-element groups, aligned as there, x_out2 only under CFG, a 2- or 4-byte dtype pair --, its
   form is LIN1, TWO or MS3, it has neither DPM_F_NOISE nor DPM_F_THRESH, mask, blend_a and blend_b (which may be NULL: blend_a
   is blended in as it is) are 16-byte aligned, mask_period is a multiple of 8 and n a multiple of mask_period.  Such requests
   form groups of their own -- never with a request without the blend -- that agree on dtypes, n, batch, model type, guidance
   kind and DPM_F_TO_X0; the three forms, blend_b NULL and not NULL, and every mask_period share a group (a row whose period is a
   multiple of 2048 takes the split tile layout of a 4-byte state, a row next to it with period 8 does not: per row,
   wave-uniform).  Every group, from ONE member on, is one run of rows and ONE launch, the runs in the order the groups open,
   among those of the other families.  Behind the rows -- and behind the n_req noise records a DPM_TABLE_NOISE call has room
   for -- the table holds one blend record per row: the record of table row i (counted over all runs) is the
   DPM_TABLE_BLEND_BYTES bytes at
     dpm_sizeof(DPM_SIZEOF_TABLE_HEADER) + n_req * dpm_sizeof(DPM_SIZEOF_TABLE_ROW)
       + (DPM_TABLE_NOISE set ? n_req * DPM_TABLE_NOISE_BYTES : 0) + DPM_TABLE_BLEND_BYTES * i
   so the two record sections never overlap and each keeps its own index; the table is dpm_sizeof(DPM_SIZEOF_TABLE_HEADER) +
   n_req * (dpm_sizeof(DPM_SIZEOF_TABLE_ROW) + [DPM_TABLE_NOISE_BYTES] + [DPM_TABLE_BLEND_BYTES]) bytes.  A record is three
   device pointers -- mask, blend_a, blend_b of the request's dpm_buffers --, the 64-bit mask_period, the bits of
   st[r].blend_alpha and st[r].blend_sigma, and two zero words.  FILL writes the records of blend rows only and leaves every
   other byte of the section untouched; LAUNCH reads them in place (scalar loads) and writes nothing to the table.  A
   DPM_F_BLEND request that does not qualify (a DPM_FORM_DENOISE stage, a period that is no multiple of 8, a misaligned mask,
   DPM_F_NOISE or DPM_F_THRESH next to the blend ...) goes, in the same call, as its own dpm_stage_launch, which blends too:
   the same bits, one more launch.  Without the flag every call is version 210's.  Every request gets the bits of its own
   dpm_stage_launch.
   Rescale rows (version 213): DPM_TABLE_RESCALE OR-ed onto either mode, alone or with any of the three flags above, makes the
   same tick with guidance-rescale stages (DPM_F_CFG_RESCALE) in the table (stage_rescale_kernel_table: the kernel of the
   request's own launch, one workgroup of 512 threads per sample, with pointers and stage scalars read from the sample's row;
   no cluster, no workspace, no wait on another workgroup).  A DPM_F_CFG_RESCALE request owns a row when dpm_stage_launch
   accepts the flag on it -- classifier-free guidance, samples of at least 2 elements, phi in (0, 1], no DPM_F_THRESH /
   DPM_F_BLEND / DPM_F_NOISE, no DPM_FORM_UNIPC, a 2- or 4-byte dtype pair, a dense network output -- and its form is LIN1, TWO,
   MS3 or DPM_FORM_DENOISE (the last stage of denoise_to_zero, its buffers checked as LIN1's), its evaluation state is its
   state, its SAMPLE, n / batch elements, is whole 8-element groups (so a multiple of 16 bytes in either dtype: the kernel
   works per sample, in 16-byte accesses), and every buffer, x_out2 included, is 16-byte aligned.  Such requests form groups of
   their own that agree on dtypes, n, batch, model type, guidance kind and DPM_F_TO_X0; the four forms, every phi
   (dpm_stage.cg_scale) and guidance scale (cfg_scale), DPM_F_STORE_M and the duplicate store share a group: each is the row's
   own.  Every group, from ONE member on, is one run of rows and ONE launch (below 2^31 samples), the runs in the order the
   groups open, among those of the other families.  A rescale row is a row like any other -- the 8 pointers and the 20 words of
   stage scalars; rows of other requests, the row size and the record sections are byte for byte those of version 211, and
   there is no further section.  A DPM_F_CFG_RESCALE request that does not qualify (a sample of 12 elements, a misaligned
   buffer, a separate evaluation state ...) goes, in the same call, as its own dpm_stage_launch, which rescales too: the same
   bits, one more launch.  Without the flag every call is version 212's.  Every sample gets the bits of its request's own
   dpm_stage_launch.
   APG rows (version 215): DPM_TABLE_APG OR-ed onto either mode, alone or with any of the four flags above, makes the same tick
   with adaptive-projected-guidance stages (DPM_F_CFG_APG) in the table (stage_apg_kernel_table: the kernel of the request's
   own launch, one workgroup of 512 threads per sample, with pointers and stage scalars read from the sample's row and its
   record; no cluster, no workspace, no wait on another workgroup).
   Where the running average lives in such a call: bs[0].workspace is the table, and in a pool any request may be request 0, so
   in a call that carries DPM_TABLE_APG -- FILL or LAUNCH -- the running average of EVERY DPM_F_CFG_APG request with beta != 0 is
   its dpm_buffers.thr_hint (n fp32 values, as workspace holds them elsewhere), whether the request owns a row or goes as its
   own launch in the same call; workspace is not read for it.  A request launched on its own inside such a call is launched
   with a copy of its buffers whose workspace is its thr_hint.  beta != 0 with a null thr_hint is DPM_ERR_ARG: nothing is
   launched, no byte written.  The refusal of a DPM_F_CFG_APG momentum in st[0] does not apply to such a call.  Without the flag
   every rule of version 214 stands: workspace is the average, and the refusal applies.
   A DPM_F_CFG_APG request owns a row when dpm_stage_launch accepts the flag on it -- classifier-free guidance and DPM_F_TO_X0,
   eta in [0, 1], r >= 0, beta in (-1, 1), no DPM_F_THRESH / DPM_F_BLEND / DPM_F_NOISE / DPM_F_CFG_RESCALE, no DPM_FORM_UNIPC, a
   2- or 4-byte dtype pair, a dense network output -- and its form is LIN1, TWO, MS3 or DPM_FORM_DENOISE, its evaluation state
   is its state, its SAMPLE, n / batch elements, is whole 8-element groups (a multiple of 16 bytes in either dtype), and every
   buffer, x_out2 included and with beta != 0 the average too, is 16-byte aligned.  Such requests form groups of their own that
   agree on dtypes, n, batch, model type, guidance kind and DPM_F_TO_X0; the four forms, eta, r, beta (rows with and without a
   momentum), the guidance scale, DPM_F_STORE_M and the duplicate store share a group: each is the row's own.  Every group,
   from ONE member on, is one run of rows and ONE launch (below 2^31 samples), the runs in the order the groups open, among
   those of the other families.  Behind the rows -- behind the n_req noise records a DPM_TABLE_NOISE call has room for and
   behind the n_req blend records of a DPM_TABLE_BLEND call -- the table holds one APG record per row: the record of table row
   i (counted over all runs) is the DPM_TABLE_APG_BYTES bytes at
     dpm_sizeof(DPM_SIZEOF_TABLE_HEADER) + n_req * dpm_sizeof(DPM_SIZEOF_TABLE_ROW)
       + (DPM_TABLE_NOISE set ? n_req * DPM_TABLE_NOISE_BYTES : 0) + (DPM_TABLE_BLEND set ? n_req * DPM_TABLE_BLEND_BYTES : 0)
       + DPM_TABLE_APG_BYTES * i
   so the record sections never overlap and each keeps its own index; the table is dpm_sizeof(DPM_SIZEOF_TABLE_HEADER) + n_req
   * (dpm_sizeof(DPM_SIZEOF_TABLE_ROW) + [DPM_TABLE_NOISE_BYTES] + [DPM_TABLE_BLEND_BYTES] + [DPM_TABLE_APG_BYTES]) bytes.  A
   record is one device pointer -- the running average, thr_hint of the request's dpm_buffers, NULL when beta == 0 --, the bits
   of eta, r and beta (st[r].cg_scale / thr_ratio / thr_max: the row's stage scalars do not carry them under the flag), and
   three zero words.  Each sample of a row advances its own slice of the row's average (sample k: the P values from k * P on).
   FILL writes the records of APG rows only and leaves every other byte of the section untouched; LAUNCH reads them in place
   (scalar loads) and writes nothing to the table.  A DPM_F_CFG_APG request that does not qualify (a sample of 12 elements, a
   misaligned buffer or average, a separate evaluation state ...) goes, in the same call, as its own dpm_stage_launch, which
   projects too: the same bits, one more launch.  Every sample gets the bits of its request's own dpm_stage_launch (with the
   average in workspace).
   CFG-Zero* rows (version 217): DPM_TABLE_ZSTAR OR-ed onto either mode, alone or with any of the five flags above, makes the
   same tick with CFG-Zero* stages (DPM_F_CFG_ZSTAR) in the table (stage_zstar_kernel_table: the kernel of the request's own
   launch, one workgroup of 512 threads per sample, with pointers and stage scalars read from the sample's row; no cluster, no
   workspace, no wait on another workgroup).  A DPM_F_CFG_ZSTAR request owns a row when dpm_stage_launch accepts the flag on it
   -- classifier-free guidance, no DPM_F_THRESH / DPM_F_BLEND / DPM_F_NOISE / DPM_F_CFG_RESCALE / DPM_F_CFG_APG, no
   DPM_FORM_UNIPC, a 2- or 4-byte dtype pair, a dense network output -- and its form is LIN1, TWO, MS3 or DPM_FORM_DENOISE (the
   last stage of denoise_to_zero, its buffers checked as LIN1's), its evaluation state is its state, its SAMPLE, n / batch
   elements, is whole 8-element groups (so a multiple of 16 bytes in either dtype: the kernel works per sample, in 16-byte
   accesses), and every buffer, x_out2 included, is 16-byte aligned.  Such requests form groups of their own that agree on
   dtypes, n, batch, model type, guidance kind and DPM_F_TO_X0; the four forms, every guidance scale (cfg_scale),
   DPM_F_STORE_M and the duplicate store share a group: each is the row's own.  Every group, from ONE member on, is one run of
   rows and ONE launch (below 2^31 samples), the runs in the order the groups open, among those of the other families.  A
   CFG-Zero* row is a row like any other -- the 8 pointers and the 20 words of stage scalars, whose flags word carries
   DPM_F_CFG_ZSTAR as the stage record does; rows of other requests, the row size and the record sections are byte for byte
   those of version 215, there is no further section, and the size of the table does not depend on the flag.  A
   DPM_F_CFG_ZSTAR request that does not qualify (a sample of 12 elements, a misaligned buffer, a separate evaluation state ...)
   goes, in the same call, as its own dpm_stage_launch, which projects too: the same bits, one more launch.  Without the flag
   every call is version 216's.  Every sample gets the bits of its request's own dpm_stage_launch.
   Two-condition rows (version 219): DPM_TABLE_PAIR OR-ed onto either mode, alone or with any of the six flags above, makes the
   same tick with stages under guidance over two conditions (DPM_GUIDE_CFG2) in the table (stage_pair_kernel_table: the
   arithmetic of the request's own stage_pair_kernel launch on 16-byte accesses, in the plain table family's launch shape -- one
   super-tile per 256-lane group, no loop, the XCD-contiguous remap --, pointers and stage scalars read from the row, the third
   output and the third copy from its pair record).  A DPM_GUIDE_CFG2 request owns a row when dpm_stage_launch accepts the
   guidance on it -- finite s1 and s2, no DPM_F_THRESH / DPM_F_BLEND / DPM_F_NOISE / DPM_F_USER_X0, no DPM_FORM_UNIPC and none
   of its flags, a 2- or 4-byte dtype pair, a dense network output -- and its form is LIN1, TWO, MS3 or DPM_FORM_DENOISE, its
   evaluation state is its state, n is a positive multiple of 8, e0, e1, g and x_out are set, and every buffer -- x_out2 and the
   third copy included -- is 16-byte aligned.  Such requests form groups of their own that agree on dtypes, n, batch, model type,
   guidance kind and DPM_F_TO_X0; the four forms, both scales, DPM_F_STORE_M and rows with and without the copies share a group:
   each is the row's own.  Every group, from ONE member on, is one run of rows and ONE launch, the runs in the order the groups
   open, among those of the other families.
   The copies: in a call that carries DPM_TABLE_PAIR -- FILL or LAUNCH -- a DPM_GUIDE_CFG2 request may carry x_out2, the second
   copy of x_out, and then carries the THIRD copy in dpm_buffers.thr_hint (n values of the state dtype; the guidance excludes
   DPM_F_THRESH, so such a stage reads no hint): the network's next input is three copies of the state.  One of the two
   without the other is DPM_ERR_ARG ("stage_launch_multi: DPM_GUIDE_CFG2 in a DPM_TABLE_PAIR call needs x_out2 and the third
   copy (dpm_buffers.thr_hint) both set or both null").  A DPM_GUIDE_CFG2 request that carries them and owns no row
   (misaligned, n no multiple of 8, multi_fuse off ...) is DPM_ERR_UNSUPPORTED with the text of version 218 ("stage_launch:
   DPM_GUIDE_CFG2 with x_out2 (the kernel has no second store)"): every request is checked before anything is written or
   launched.  A DPM_GUIDE_CFG2 request without copies that owns no row goes, in the same call, as its own dpm_stage_launch.
   The pair records follow the rows and the noise, blend and APG records of the flags present; record i (counted over all runs)
   is the DPM_TABLE_PAIR_BYTES bytes at
     dpm_sizeof(DPM_SIZEOF_TABLE_HEADER) + n_req * dpm_sizeof(DPM_SIZEOF_TABLE_ROW)
       + (DPM_TABLE_NOISE ? n_req * DPM_TABLE_NOISE_BYTES : 0) + (DPM_TABLE_BLEND ? n_req * DPM_TABLE_BLEND_BYTES : 0)
       + (DPM_TABLE_APG ? n_req * DPM_TABLE_APG_BYTES : 0)
       + DPM_TABLE_PAIR_BYTES * i
   (the section is present under DPM_TABLE_PAIR or, from version 221, DPM_TABLE_PERP) and the table is dpm_sizeof(DPM_SIZEOF_TABLE_HEADER) + n_req * (dpm_sizeof(DPM_SIZEOF_TABLE_ROW) + [DPM_TABLE_NOISE_BYTES] +
   [DPM_TABLE_BLEND_BYTES] + [DPM_TABLE_APG_BYTES] + [DPM_TABLE_PAIR_BYTES]) bytes.  A record is two device pointers: g of the
   request's dpm_buffers, then its thr_hint (NULL: no copies).  The row is a row like any other: 8 pointers (x_out2 the eighth)
   and the 20 words of stage scalars, s1 in cfg_scale, s2 in cg_scale.  FILL leaves the pair-record slots of rows of other kinds
   untouched.  Without the flag every call is version 218's: x_out2 on a DPM_GUIDE_CFG2 request is refused, thr_hint is not
   read, and such a request owns no row.  Every element gets the bits of its request's own dpm_stage_launch.
   Perp-Neg rows (version 221): DPM_TABLE_PERP OR-ed onto either mode, alone or with any of the seven flags above, makes the
   same tick with Perp-Neg stages (DPM_F_CFG2_PERP on a DPM_GUIDE_CFG2 record) in the table (stage_perp_kernel_table: the
   kernel of the request's own launch, one workgroup of 512 threads per sample, with pointers and stage scalars read from the
   sample's row, the third output and the third copy from its pair record; no cluster, no workspace, no wait on another
   workgroup).  A flagged request owns a row when dpm_stage_launch accepts it -- finite s and w, no DPM_F_THRESH / DPM_F_BLEND /
   DPM_F_NOISE / DPM_F_USER_X0, no DPM_FORM_UNIPC and none of its flags, a 2- or 4-byte dtype pair, a dense network output --
   and its form is LIN1, TWO, MS3 or DPM_FORM_DENOISE, its evaluation state is its state, its SAMPLE, n / batch elements, is
   whole 8-element groups (so a multiple of 16 bytes in either dtype: the kernel works per sample, in 16-byte accesses), e0,
   e1, g and x_out are set, and every buffer -- x_out2 and the third copy included -- is 16-byte aligned.  Such requests form
   groups of their own that agree on dtypes, n, batch, model type, guidance kind and DPM_F_TO_X0; the four forms, both scales,
   DPM_F_STORE_M and rows with and without the copies share a group: each is the row's own.  Every group, from ONE member on,
   is one run of rows and ONE launch (below 2^31 samples), the runs in the order the groups open, among those of the other
   families.  A flagged request never owns a two-condition row: in a DPM_TABLE_PAIR | DPM_TABLE_PERP call one that does not
   qualify here (a sample of 12 elements, a misaligned buffer ...) goes, in the same call, as its own dpm_stage_launch
   (stage_perp_kernel), as it does in mode 0: the same bits, one more launch.
   The record is the pair record of version 219 -- g, then thr_hint (NULL: no copies) -- in the same section at the same
   offset: the section is present when the call carries DPM_TABLE_PAIR or DPM_TABLE_PERP or both, n_req records either way, and
   the table's size counts [DPM_TABLE_PAIR_BYTES] once under either flag.  For a table_mode without DPM_TABLE_PERP offsets and
   size are those of version 219.  The copies follow the rules above: in a call that carries DPM_TABLE_PERP a flagged
   DPM_GUIDE_CFG2 request may carry x_out2 and then the THIRD copy in dpm_buffers.thr_hint; one without the other is
   DPM_ERR_ARG with the text above (it names DPM_TABLE_PERP in place of DPM_TABLE_PAIR when the call carries only that flag);
   copies on a request that owns neither a pair row nor a Perp-Neg row are DPM_ERR_UNSUPPORTED ("stage_launch: DPM_GUIDE_CFG2
   with x_out2 (the kernel has no second store)"); every request is checked before anything is written or launched.  The
   kernel stores the state to x_out and, where the row carries the copies, to both of them, each advanced to the workgroup's
   sample.  Without the flag every call is version 220's: a DPM_F_CFG2_PERP request in a table-mode call is refused
   ("stage_launch_multi: DPM_F_CFG2_PERP in a table-mode call (the table's rows have no per-sample pass)").  Every sample gets
   the bits of its request's own dpm_stage_launch.
   Any other table_mode (valid: DPM_TABLE_FILL or DPM_TABLE_LAUNCH, plus any of DPM_TABLE_NOISE, DPM_TABLE_THRESH, DPM_TABLE_BLEND,
   DPM_TABLE_RESCALE, DPM_TABLE_APG, DPM_TABLE_ZSTAR, DPM_TABLE_PAIR, DPM_TABLE_PERP: 1, 2, 5, 6, 9, 10, 13, 14, 33, 34, 37, 38, 41, 42, 45, 46,
   each of those plus 128, each of all these plus 512 -- the 64 modes of version 215 --, each of those 64 plus 4096 -- the 128
   modes of version 217 --, each of those 128 plus 16384 -- the 256 modes of version 219 --, and each of those 256 plus 65536; bits 16, 64, 256, 1024, 2048,
   8192 and 32768 are unassigned), a non-zero
   one without per_request_stages, or with fuse_shapes == 1:
   DPM_ERR_ARG. */
#define DPM_MULTI_MAX 32
DPM_API int dpm_stage_launch_multi(const dpm_stage* st, const dpm_buffers* bs, int n_req, void* stream);
/* scratch needed by stages with DPM_F_THRESH on the current device: 0 when one workgroup per sample is the plan (the
   sample lives in that workgroup's LDS), else ~45-80 KiB per sample of slots, histograms and counters through which the
   workgroup cluster of a sample exchanges its candidates (small batches, samples beyond 12288 elements).
   Pass it as dpm_buffers.workspace.  Contract: the caller ZERO-FILLS the workspace once (hipMemset) before its first use;
   every launch leaves it zero-filled again (the last workgroup of a cluster cleans up), so no launch pays for a clear.
   Launches that share a workspace must be ordered (same stream).
   Cluster waits are bounded (dpm_launch_opts.thr_spin_limit polls, milliseconds).  When the peers of a cluster are kept off the
   chip that long -- another process running clusters on the same GPU, two clustered graphs replayed concurrently -- the
   waiting workgroup gives up, computes the order statistics of its sample alone from global memory and carries on:
   the launch's results are the same bits, the workspace is left zero-filled as always, nothing is reported as an error. */
DPM_API size_t dpm_threshold_workspace_bytes(int64_t batch, int64_t per_sample);
/* diagnostics: 1 when a cluster wait of any clustered thresholding launch of this process timed out (and was recovered
   from) since the last call, else 0.  Reads and clears a host-mapped word; meaningful after the launches in question
   have completed (no synchronisation here). */
DPM_API int dpm_cluster_timeout_poll(void);
#define DPM_THR_HINT_WORDS 4   /* floats per sample of dpm_buffers.thr_hint / dpm_run_buffers.thr_hint */
/* x_t = alpha_t*x + sigma_t*noise for nt times (add_noise, ref :1012-1030); out is [nt, n] */
DPM_API int dpm_add_noise_launch(const dpm_schedule* s, const float* t_host, int nt, const void* x, const void* noise,
                         void* out, int64_t n, int dtype, void* stream);
/* the same with DOUBLE times on double tensors (version 201): alpha_t / sigma_t evaluated in double at the double times -- what
   the reference's type promotion makes of add_noise(x, t) when t is a double tensor or the schedule's tables are
   (NoiseScheduleVP(dtype=torch.float64)): the result is float64 whatever x was (the host converts x / noise first) */
DPM_API int dpm_add_noise_launch_f64(const dpm_schedule* s, const double* t_host, int nt, const void* x, const void* noise,
                             void* out, int64_t n, void* stream);
/* stand-alone mask blend  out = x*mask + (1-mask)*(alpha*a + sigma*b)  (b NULL: (1-mask)*a): the DPM_F_BLEND
   epilogue as its own launch, for callable use of the corrector and for x_T before the first update (ref :1180) */
DPM_API int dpm_blend_launch(const void* x, const void* mask, const void* a, const void* b, float alpha, float sigma, void* out,
                     int64_t n, int64_t mask_period, int dtype, void* stream);
/* error norm of the adaptive solver (ref :999-1001): E_b = sqrt(mean(((xh-xl)/delta)^2)) per sample in e_out[0..batch),
   and their maximum over the batch (the value the step-size controller reads) in e_out[batch] */
DPM_API int dpm_adaptive_error_launch(const void* x_lower, const void* x_higher, const void* x_prev, float atol, float rtol,
                              float* e_out /* [batch + 1] device */, int64_t batch, int64_t per_sample, int dtype,
                              void* stream);

/* ---- adaptive step-size solver with the controller ON THE DEVICE (dpm_solver_adaptive, ref :956-1010) --------------
   The reference's loop decides accept / reject and the next step size on the host from E = max_b ||(x_hi - x_lo)/delta||,
   i.e. one device -> host synchronisation per iteration.  Here the controller state (s, lambda_s, h, nfe, done) and the
   coefficients of the iteration's stages live in device memory: a one-thread kernel takes the decision of the previous
   iteration, evaluates inverse_lambda and every coefficient of the next one with the planner's own code
   (csrc/dpm_coef.hpp, compiled for the device) and fills the time vectors the network is called with; the stage kernels
   read their coefficients from there; accepted states are committed by a device-side copy.  After `done` every kernel
   of the handle is a no-op, so the host may enqueue a fixed number of iterations (hipGraph capture) or poll the
   host-mapped status words without synchronising.  One iteration =
       dpm_adaptive_begin -> [network at t_vectors[0]] -> stages ... -> dpm_adaptive_error
   with the stages of DPM-Solver-12 (order 2: which = 0 lower, 2..3 higher) or -23 (order 3: 0..1 lower, 3..4 higher;
   stage 2 equals stage 0).  The caller owns x, x_prev, x_lower, x_higher, the scratch states, the time vectors and the
   error word; the handle owns ~2 KB of device state and a copy of the schedule tables. */
typedef struct dpm_adaptive_desc {
  int32_t algorithm_type; /* DPM_ALGO_*   */
  int32_t solver_type;    /* DPM_SOLVER_* */
  int32_t order;          /* 2 or 3       */
  int32_t model_type;     /* DPM_MODEL_*  */
  int32_t guidance;       /* DPM_GUIDE_*  */
  int32_t reserved;
  double guidance_scale;
  double t_start, t_end;  /* t_T, t_0 */
  double h_init, atol, rtol, theta, t_err; /* ref :956 defaults 0.05, 0.0078, 0.05, 0.9, 1e-5 */
} dpm_adaptive_desc;
typedef struct dpm_adaptive dpm_adaptive;
DPM_API int dpm_adaptive_create(const dpm_schedule* s, const dpm_adaptive_desc* d, dpm_adaptive** out);
DPM_API void dpm_adaptive_destroy(dpm_adaptive* a);
/* static fields (form, flags, slots) of stage `which` (0..4); the float fields are placeholders */
DPM_API int dpm_adaptive_stage_template(const dpm_adaptive* a, int which, dpm_stage* out);
/* start of a run: s = t_T, h = h_init, nfe = 0 */
DPM_API int dpm_adaptive_reset(dpm_adaptive* a, void* stream);
/* decision on the previous iteration (E read from *e_dev, then cleared), commit of an accepted step
   (x <- x_higher, x_prev <- x_lower), plan of the next iteration, t_vectors[j][0 | 1][0..tv_len) <- t_eval | t_input of
   network evaluation j */
DPM_API int dpm_adaptive_begin(dpm_adaptive* a, void* x, void* x_prev, const void* x_lower, const void* x_higher, int64_t n,
                       int dtype, float* e_dev, float* t_vectors, int64_t tv_len, void* stream);
/* stage `which` of the current iteration: `st` = the caller's copy of the template (it may edit flags / model_type /
   guidance, e.g. to feed a known model value), float coefficients come from the device */
DPM_API int dpm_adaptive_stage_launch(dpm_adaptive* a, int which, const dpm_stage* st, const dpm_buffers* b, void* stream);
/* *e_dev <- max(*e_dev, max_b E_b) (ref :999-1001); several workgroups per sample, fp32 / fp16 / bf16 */
DPM_API int dpm_adaptive_error(dpm_adaptive* a, const void* x_lower, const void* x_higher, const void* x_prev, int64_t batch,
                       int64_t per_sample, int dtype, float* e_dev, void* stream);
/* host-mapped status as of the last dpm_adaptive_begin the device has executed: no synchronisation.
   done: 0 running, 1 t_end reached, 2 the run was ended by a NaN error estimate -- the begin that read it rejected the
   step, left s, h, nfe and the time vectors at their last (finite) values, and every later kernel of the handle is a
   no-op as after 1.  dpm_adaptive_done_at reports the same three values. */
DPM_API int dpm_adaptive_poll(const dpm_adaptive* a, int* done, int* nfe, int* iterations, int* accepted);
/* `done` as recorded by the begin_index-th dpm_adaptive_begin since the last reset (a ring of the last 32): the value to
   look at after waiting for THAT launch -- identical on every rank of a batch-sharded run, whatever has run since */
DPM_API int dpm_adaptive_done_at(const dpm_adaptive* a, int begin_index);

/* native sample loop for non-Python hosts and for the solver-only benchmark.
   model(user, stage, x, t_input, t_eval, e0_out, e1_out): evaluate the network on x, write the raw output(s);
   NULL means the outputs are already staged in e0/e1 (frozen model).  All buffers are the caller's:
   xbuf[0] holds x_T and is only read; xbuf[1..3] are state-sized scratch the loop rotates through;
   hist[num_slots] cache model values.  On return *result is the index of the xbuf holding the final sample. */
typedef int (*dpm_model_cb)(void* user, const dpm_stage* st, const void* x, void* e0, void* e1, void* stream);
typedef struct dpm_run_buffers {
  void* xbuf[4];
  void* hist[3];
  void* e0;
  void* e1;
  void* workspace;
  int64_t n, batch;
  int32_t state_dtype, eps_dtype;
  /* ---- optional (zero = off) ---- */
  int64_t eps_stride;  /* as dpm_buffers.eps_stride: e0 / e1 are channel slices of a wider network output        */
  int32_t dup_state;   /* 1: every xbuf holds 2n elements and each state is written to both halves, so the model
                          callback of a classifier-free-guidance network receives its [2B,...] input ready-made
                          (xbuf[0] must already hold x_T twice)                                                  */
  int32_t reserved;
  float* thr_hint;     /* as dpm_buffers.thr_hint (DPM_THR_HINT_WORDS floats per sample, or NULL)                */
  const dpm_launch_opts* opts; /* per-call options handed to every launch of the run, NULL = defaults (version 200;
                                  dpm_plan_run_multi reads rbs[0].opts)                                            */
} dpm_run_buffers;
DPM_API int dpm_plan_run(const dpm_plan* p, const dpm_run_buffers* rb, dpm_model_cb model, void* user, void* stream,
                 int* result);
/* several independent sampling requests advanced stage by stage (all requests stage s, then all stage s+1, ...)
   through dpm_stage_launch_multi: what a server holding n requests in flight does, and -- with a frozen model -- the
   HBM-cold measurement mode of bench.py: between two stages of one request the other n-1 requests stream their buffers
   through the 256 MiB Infinity Cache.  All requests must share n, batch and dtypes.  ms (optional,
   [n_req * num_stages], request-major) receives kernel-only durations; a fused launch's duration is divided evenly
   over the requests it advanced (with n_req = 1: the kernel-only durations of one frozen-model trajectory).
   dpm_launch_opts.no_fuse launches request by request instead. */
DPM_API int dpm_plan_run_multi(const dpm_plan* p, const dpm_run_buffers* rbs, int n_req, void* stream, float* ms, int* results);

/* ---- hipGraph capture of a whole trajectory ------------------------------------------------------------
   The step loop is launch-bound between network calls (a stage kernel runs for microseconds): capture the plan's
   launches over fixed buffers once, replay with a single hipGraphLaunch per trajectory.  `stream` must be a real
   (non-null) stream; `model` as in dpm_plan_run -- everything it does must be capturable (enqueue-only on `stream`);
   NULL = frozen outputs already staged in e0/e1.  The buffers named by `rb` are baked into the graph. */
typedef struct dpm_graph dpm_graph;
DPM_API int dpm_graph_create(const dpm_plan* p, const dpm_run_buffers* rb, dpm_model_cb model, void* user, void* stream,
                     dpm_graph** out);
DPM_API int dpm_graph_launch(dpm_graph* g, void* stream);
DPM_API int dpm_graph_result(const dpm_graph* g);    /* index of the xbuf that holds the final sample            */
DPM_API int dpm_graph_num_nodes(const dpm_graph* g); /* kernel / memset nodes captured                           */
DPM_API void dpm_graph_destroy(dpm_graph* g);

/* ---- misc ---------------------------------------------------------------------------------- */
DPM_API int dpm_version(void);
/* sizeof() of the ABI structs as compiled, so a binding can verify its own layout at load time */
enum { DPM_SIZEOF_STAGE = 0, DPM_SIZEOF_BUFFERS = 1, DPM_SIZEOF_PLAN_DESC = 2, DPM_SIZEOF_RUN_BUFFERS = 3,
       DPM_SIZEOF_ADAPTIVE_DESC = 4, DPM_SIZEOF_LAUNCH_OPTS = 5, DPM_SIZEOF_STAGE_F64 = 6,
       DPM_SIZEOF_TABLE_HEADER = 7, DPM_SIZEOF_TABLE_ROW = 8 /* version 208: the table of dpm_launch_opts.table_mode */,
       DPM_SIZEOF_TABLE_NOISE = 10 /* version 209: a noise record of a DPM_TABLE_NOISE table (9 is unassigned: 0) */,
       DPM_SIZEOF_TABLE_BLEND = 12 /* version 211: a blend record of a DPM_TABLE_BLEND table (11 is unassigned: 0) */,
       DPM_SIZEOF_TABLE_APG = 14 /* version 215: an APG record of a DPM_TABLE_APG table (13 is unassigned: 0) */,
       DPM_SIZEOF_TABLE_PAIR = 18 /* version 219: a pair record of a DPM_TABLE_PAIR table (15, 16 and 17 are unassigned: 0 --
                                     the CFG-Zero* rows of version 217 have no record, and 16 is pinned as 0 since then) */ };
DPM_API size_t dpm_sizeof(int which);
DPM_API const char* dpm_last_error(void); /* thread-local text of the last non-zero return */
DPM_API int dpm_device_info(int* n_cu, int* lds_bytes, char* arch, int arch_len);

#ifdef __cplusplus
}
#endif
#endif /* DPM_HIP_H */
