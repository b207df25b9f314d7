/* libspart_hip.so -- C ABI of the MI355X-native batched SPART evaluator.
 *
 * The reference (wirrell/SPART-python) has no FFI layer: its hot path is the five plain
 * Python callables
 *     BSM(soilpar, optical_params)                  src/SPART/bsm.py:17
 *     PROSPECT_5D(leafbio, optical_params)          src/SPART/prospect_5d.py:117
 *     SAILH(soil, leafopt, canopy, angles)          src/SPART/sailh.py:14
 *     SMAC(angles, atm, coefs)                      src/SPART/smac.py:14
 *     SPART(...).run()                              src/SPART/SPART.py:162
 * Each entry point below replaces the arithmetic of one of them for a BATCH of B samples;
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every array pointer is DEVICE memory owned by the caller (e.g. a torch tensor's
 *     data_ptr()); the library allocates only its context and never frees caller memory;
 *   - per-sample inputs are structure-of-arrays, float64, length B (sample-level geometry is
 *     always computed in float64);
 *   - spectra and result columns are row-major (B, nbands), band-contiguous, in `dtype`; the row pitch of the
 *     2162- / 2001-wide spectrum arrays is the row width unless spart_ctx_set_row_pitch says otherwise;
 *   - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous on it (spart_run_batch may run some
 *     of its kernels on a side stream the context owns -- one per caller stream, for the first 32 caller streams a context
 *     sees; calls on further streams run every kernel on `stream` itself: same results, no overlap -- and joins them back
 *     into `stream` before it returns, so the caller sees plain stream semantics, HIP-graph capture included);
 *   - a context is THREAD-SAFE: its tables are immutable after creation and the little per-call state it has (side
 *     streams, events) is guarded, so any number of host threads may call into one context on any streams.  Calls
 *     that run concurrently on the GPU (different streams) need different workspaces; if two streams do pass the
 *     same workspace, the later call is ordered after the earlier one (hipStreamWaitEvent on its completion) -- slow,
 *     never a race, for any number of (workspace, stream) pairs: the context remembers every use until it has seen
 *     it complete -- or fails with SPART_ERR_INVALID when that order cannot be expressed (e.g. across a stream
 *     capture).  HIP-graph REPLAYS are outside the library's view: a captured call's workspace belongs to its graph.  The
 *     first call on a stream (and the first use of a workspace on it) creates that stream's side stream / events: issue
 *     one ordinary call on the stream before capturing it, so that the capture itself creates nothing;
 *   - return value 0 = ok, <0 = error (spart_last_error gives the text).  Numerical trouble
 *     propagates as NaN/inf exactly like the reference (no clamping).
 */
#ifndef SPART_HIP_H
#define SPART_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPART_NWL 2001      /* 400..2400 nm            (SPART.py:303)      */
#define SPART_NWLS 2162     /* + 161 thermal bands      (SPART.py:307-310)  */
#define SPART_NLINCL 13     /* leaf inclination classes (sailh.py:346)      */
#define SPART_NPARAM 27     /* parameter columns of spart_run_batch         */
#define SPART_NCOEF 48      /* SMAC coefficient rows    (smac.py:44-92)     */

#define SPART_NLAYERS 60    /* canopy layers, CanopyStructure's default (sailh.py:345) */
#define SPART_MAX_NLAYERS 1000000

/* Version of THIS interface (struct layouts, argument lists, stage count): spart_abi_version() of a loaded library must
 * equal the header's a binding was written against (the Python loader checks, so that a library built from another
 * round's header -- e.g. through SPART_HIP_LIB -- is refused instead of being called with shifted arguments).
 *   6: spart_materialize.lidf_in / .nlayers, spart_sailh_batch(lidf_in, nlayers), spart_abi_version itself
 *   7: spart_workspace_bandsum
 *   8: spart_lut_topk, spart_lut_topk_workspace_bytes, spart_lut_topk_stats
 *   9: spart_lut_topk_wide, spart_lut_topk_wide_workspace_bytes, spart_lut_topk_wide_stats; sensors of up to SPART_NWLS bands
 *  10: spart_lut_topk_obs_weights, spart_lut_topk_obs_weights_workspace_bytes, spart_lut_topk_obs_weights_stats
 *  11: spart_lut_summarise
 *  12: spart_srf_support; spart_materialize.R_TOC_srf ... rdd_srf
 *  13: spart_refine, spart_refine_workspace_bytes, spart_refine_opt
 *  14: spart_refine_opt.prior_per_obs, prior_mean, prior_weight
 * spart_refine_srf was added WITHOUT a new number: it is one more symbol, no struct layout or argument list changed, so every
 * caller of version 14 still calls what it called; a binding that needs the symbol looks it up when it loads the library.
 * spart_refine_views, spart_views_workspace_bytes and spart_refine_views_opt were added by the same rule: new symbols
 * and a new struct that embeds spart_refine_opt unchanged.  spart_refine_posterior and spart_posterior_out likewise, and
 * spart_lut_bayes, spart_lut_bayes_workspace_bytes and spart_lut_bayes_stats with spart_lut_bayes_opt / _out.
 * spart_refine_tiles and spart_tiles_workspace_bytes with spart_refine_tiles_opt / spart_tiles_out came by that rule too,
 * and spart_lut_bayes_quantiles with spart_lut_bayes_q_opt / _q_out, which embed spart_lut_bayes_opt / _out unchanged.  spart_products with spart_products_out likewise.
 * spart_refine_series and spart_series_workspace_bytes with spart_refine_series_opt, which embeds spart_refine_tiles_opt
 * unchanged, likewise.  spart_sobol and spart_sobol_workspace_bytes with spart_sobol_opt / spart_sobol_out likewise, and
 * spart_sample and spart_sample_workspace_bytes with spart_sample_opt / spart_sample_out.  spart_refine_mix and
 * spart_mix_workspace_bytes with spart_refine_mix_opt, which embeds spart_refine_opt unchanged, and spart_refine_mix_out likewise.
 * spart_vjp and spart_vjp_workspace_bytes with spart_vjp_opt likewise.  spart_refine_leaf with spart_leaf_fit_opt / _out likewise. */
#define SPART_ABI_VERSION 14

#define SPART_F32 0
#define SPART_F64 1

#define SPART_OK 0
#define SPART_ERR_INVALID (-1)    /* bad argument                          */
#define SPART_ERR_HIP (-2)        /* HIP runtime error                     */
#define SPART_ERR_WORKSPACE (-3)  /* workspace missing or too small        */
#define SPART_ERR_NOSENSOR (-4)   /* context was created without a sensor  */

typedef struct spart_ctx spart_ctx;

/* Static tables, HOST pointers, float64; copied to the device by spart_ctx_create.
 * Spectral tables are the arrays of the reference's optical_params.pkl / ET_irradiance.pkl
 * (SPART.py:399-416), length 2001; the sensor block is sensor_information/<sensor>.pkl
 * (SPART.py:419-424): keys wl_smac, SMAC_coef, wl_srf_smac, p_srf_smac.  nb = 0 builds a
 * context without sensor (leaf / soil / canopy entry points only). */
typedef struct spart_tables {
  const double *nr, *Kab, *Kca, *Kdm, *Kw, *Ks, *Kant, *cbc, *prot; /* prospect_5d.py:158-167 */
  const double *GSV;                                                /* (2001,3) row-major, bsm.py:45 */
  const double *nw;                                                 /* bsm.py:55 */
  const double *Ea;                                                 /* SPART.py:181 */
  int32_t nb;                                                       /* sensor bands, 0 ... SPART_NWLS (2162: one per evaluation
                                                                       band of the model, thermal ones included); any centres */
  const double *wl_smac;                                            /* (nb,) band centres, nm */
  const double *coef;                                               /* (48, nb) row-major, rows in smac.py:44-92 order
                                                                       (ah2o nh2o ao3 no3 ao2 no2 po2 aco2 nco2 pco2 ach4 nch4 pch4
                                                                       ano2 nno2 pno2 aco nco pco a0s a1s a2s a3s a0T a1T a2T a3T taur
                                                                       a0taup a1taup wo gc a0P a1P a2P a3P a4P Rest1..4 Resr1..3 Resa1..4) */
  int32_t nsrf;                                                     /* SRF samples per band */
  const double *wl_srf;                                             /* (nsrf, nb) row-major, NaN padded */
  const double *p_srf;                                              /* (nsrf, nb) row-major */
} spart_tables;

/* Optional full-spectrum outputs of spart_run_batch (the reference object's soilopt /
 * leafopt / canopyopt attributes, SPART.py:66-81) and evaluation options.  NULL members are skipped;
 * passing opt = NULL means: columns only, all bands evaluated. */
typedef struct spart_materialize {
  void *leaf_refl, *leaf_tran; /* (B,2162) thermal-padded, SPART.py:445-470 */
  void *leaf_kchl;             /* (B,2001) kChlrel, prospect_5d.py:197-198   */
  void *soil_refl;             /* (B,2162) wet soil, padded SPART.py:427-442 */
  void *soil_refl_dry;         /* (B,2001)                                    */
  void *rso, *rdo, *rsd, *rdd; /* (B,2162) sailh.py:224-233                  */
  void *rsoil;                 /* (B,nb) debug column, SPART.py:262-267      */
  void *La;                    /* (B,nb) convolved ET radiance, SPART.py:183 */
  const void *rdry_in;         /* INPUT, optional: (B,2001) user dry-soil spectra in `dtype` (SoilParametersFromFile,
                                  bsm.py:42-43, 155-199); params[9..11] (B, lat, lon) may then be NULL */
  void *band_mean;             /* (4,2162) batch means of rso, rdo, rsd, rdd (LUT summary; no reference counterpart) */
  int32_t prune_unused_bands;  /* R_TOC / R_TOA / L_TOA (and rsoil) ALWAYS come from the <= 2 nb spectral bands they depend on
                                  (np.interp support points, SPART.py:220-223): prelude -> column kernel.
                                  0 (default): beside that, every one of the 2162 bands of every sample is evaluated by the
                                  fused full-band kernel (band sums / band_mean / the spectra requested above); 1: that
                                  kernel only runs for requested spectra -- identical columns (the same kernels produce
                                  them), the work is not "full spectra" */
  int32_t f32_columns;         /* dtype SPART_F32 only.  0 (default): the column path (prelude constants, the canopy model at
                                  the sensor bands, SMAC, TOC->TOA) is float64 whatever the dtype, so R_TOC / R_TOA / L_TOA are the float64
                                  mode's values rounded once to float32 (the 1e-4 contract then also holds for nearly
                                  conservative PROSPECT-PRO leaves, where the reference's canopy formulas cancel,
                                  sailh.py:185-214); materialised spectra and band_mean are float32 arithmetic.
                                  1: the canopy model at the sensor bands is evaluated in float32 as well (fast prelude) */
  int32_t f32_bands;           /* dtype SPART_F64 only.  1: R_TOC / R_TOA / L_TOA (and rsoil, La) are float64 and IDENTICAL
                                  to the float64 mode's -- they come from the same float64 column path -- while the
                                  evaluation of all 2162 bands of every sample (the band sums) runs in float32.
                                  Materialised spectra, band_mean and rdry_in cannot be combined with it (SPART_ERR_INVALID). */
  int32_t fast_prelude;        /* 0 (default): the reference's own LIDF fixed-point iteration with its |dx| <= 1e-8 stopping rule
                                  (sailh.py:378-382) and 10-point hot-spot panels -- the columns agree with the reference to
                                  ~1e-11.  1: the ROOT of the same equation by Newton (the reference stops up to ~5e-8 short
                                  of it) and 8-point panels; the per-sample prelude kernel takes 0.41 instead of 0.69 ms
                                  per 1M spectra (round 5; 0.45 / 0.93 when this option was introduced).  It is a different function at the 1e-8 level.  Measured over all 2 x 13M
                                  float64 column entries of BASELINE configs 4 and 5 (1M rows each; bench.py
                                  configs.fast_prelude.float64_columns_vs_default and test_fast_prelude_at_size repeat the
                                  measurement): on SURVEY 8(d)'s metric |d| / max(|ref|, 1e-6) the median is 2.5e-10, 99.999 % of
                                  the entries of R_TOC / R_TOA / L_TOA are within 1.5e-7, and 15 + 27 of the 2 x 13M R_TOC
                                  entries exceed 1e-6 (maximum 1.7e-5) -- every one of them an entry whose own magnitude is
                                  below 1e-3 (strongly absorbing bands, |d| < 1e-9).  So: inside the float32 contract (1e-4)
                                  everywhere, inside the float64 contract (1e-6) wherever the value is at least 1e-3.
                                  Implied by f32_columns */
  const double *lidf_in;       /* INPUT, optional: (B,13) float64 row-major, the leaf inclination distribution the reference's
                                  SAILH reads from canopy.lidf at call time (sailh.py:51 -> k, K, bf, sob, sof at :93-97).  NULL
                                  (default): derived from params[16..17] = LIDFa, LIDFb exactly as CanopyStructure's constructor
                                  does (sailh.py:348, 351-398).  Given: used as it is (no normalisation, like the reference's
                                  dot products), LIDFa / LIDFb are not read and may be NULL */
  int32_t nlayers;             /* canopy.nlayers (sailh.py:48): 0 = the default 60.  It enters the model only as dx = 1 / nlayers,
                                  the width of the stretch below the canopy that Pso[nlayers] averages (:131-135, 219); one value
                                  per call.  1 ... SPART_MAX_NLAYERS */
  /* SRF-convolved sensor columns, (B,nb) in `dtype`, each optional.  R_TOC / R_TOA / L_TOA above sample the canopy at the
     np.interp support of the band CENTRE (SPART.py:219-223); a real band integrates its spectral response function.  These
     seven apply the reference's own convolution, calculate_spectral_convolution (SPART.py:358-396), to the four canopy
     spectra on the model grid wlS -- 2162 points: 400..2400 nm by 1, 2500..15000 by 100, 16000..50000 by 1000 -- with the
     context's wl_srf / p_srf (the tables k_econv already convolves the irradiance with):
       idx[i,j] = the grid point nearest to wl_srf[i,j] in exact arithmetic; ties to the lower index (2450 nm -> index 2000);
                  NaN -> 0.  This is the reference's np.argmin(np.abs(wlS - w)) for every |w| < 1e15; beyond that the
                  reference's float64 subtraction no longer tells the grid points apart and it returns 0, where this library
                  keeps the nearest point (index 0 for a huge negative w, as the reference; the last one for a huge positive
                  w).  The packaged tables hold such wavelengths only with weights <= 7e-310, and one of them is positive:
                  Sentinel-2B band 4 has a sample at +9.1e306 nm, which goes to the thermal evaluation here and to index 0
                  in the reference, so that band's support has one entry more (963 in all, where the literal argmin
                  gives 962).
       ev = min(idx, 2001): the 161 thermal pad bands are the one thermal evaluation, as everywhere in this library.
       For band j: E_j = the ascending list of distinct ev; q_e = the sum of p_srf[i,j] over the samples that map to e and
       Q_j = sum_i p_srf[i,j], both summed in float64 in i order on the host (spart_srf_support).  Weights are used as given
       (negative ones included); zero-weight entries stay, so a NaN spectrum value propagates; a Q_j of 0 or non-finite
       propagates as the reference's division does.
       x_srf[s,j] = (sum over e in E_j, ascending, of q_e x[s,e]) / Q_j        for x = rso, rdo, rsd, rdd, all float64
     (fused multiply-adds, one accumulator per value: ONE order of summation whatever the batch).  SMAC and TOC -> TOA
     (SPART.py:243-252) then run on these four values in place of the interpolated ones, and L_TOA_srf = La R_TOA_srf with
     the La of the `La` member.  The outputs are the float64 column path rounded once to `dtype` in every mode (pruned or
     not, f32_bands, lidf_in, nlayers, rdry_in); with f32_columns they are refused (SPART_ERR_INVALID).  With all seven NULL
     nothing is launched for them.  The library does what the tables say: whether a band's SRF column belongs to its
     centre and SMAC coefficients is the caller's business (spart_amd.check_srf / align_srf). */
  void *R_TOC_srf, *R_TOA_srf, *L_TOA_srf;
  void *rso_srf, *rdo_srf, *rsd_srf, *rdd_srf;
} spart_materialize;

int spart_ctx_create(spart_ctx **out, int device, const spart_tables *tables);
int spart_ctx_destroy(spart_ctx *ctx);
const char *spart_last_error(const spart_ctx *ctx); /* text of the last error raised ON THE CALLING THREAD (ctx may be NULL) */

/* Identity of this binary: 12 hex digits over the kernel / ABI sources, compiler flags and math variant it was built
 * from (spart-python_amd/build.py: source_id).  The Python loader refuses a library whose id is not that of the
 * sources next to it, and bench.py prints it, so a stale .so cannot be measured silently.  No reference counterpart. */
const char *spart_build_id(void);
int spart_abi_version(void);                              /* SPART_ABI_VERSION the library was compiled with */

int spart_ctx_nb(const spart_ctx *ctx);                    /* sensor bands of the context */
int spart_ctx_econv(const spart_ctx *ctx, double *host_out); /* (nb,) SRF-convolved ET irradiance (SPART.py:389-394), copied to HOST */

/* Row pitch, in elements, of EVERY (B,2162) and (B,2001) spectrum array this context reads or writes (the outputs /
 * inputs of spart_prospect_batch, spart_bsm_batch, spart_sailh_batch and the spart_materialize members of
 * spart_run_batch; (B,nb) columns and band_mean stay dense).  Default = dense (2162 / 2001); 0 restores it.
 * A 2162-float row is 8648 B, so dense rows start off the 128 B line grid and the 1 KB row segments a workgroup
 * stores straddle lines: on MI355X the materialised store stream then reaches 3.3 TB/s, with rows padded to a
 * multiple of 64 elements (2176 / 2048) 5.9 TB/s (tools/ubench/write_pattern.hip).  No reference counterpart. */
int spart_ctx_set_row_pitch(spart_ctx *ctx, int64_t pitch_full, int64_t pitch_optical);

/* calculate_tav (prospect_5d.py:249-311): average transmissivity of a dielectric plane surface for the cone half-angle
 * alpha_deg and n refractive indices.  HOST function on host pointers, float64, no context and no GPU: it is the routine
 * the library derives its interface tables from in spart_ctx_create, exported so that the
 * Python mirror of the reference function runs the same arithmetic. */
int spart_calculate_tav(double alpha_deg, const double *nr, int64_t n, double *out);

/* The compressed SRF support behind spart_materialize's *_srf outputs (defined there).  HOST function on host pointers, no
 * context and no GPU: the routine spart_ctx_create itself calls.  wl_srf, p_srf: (nsrf, nb) row-major as in spart_tables.
 * start (nb + 1): band j owns entries start[j] ... start[j + 1] - 1; ev / q (start[nb]): E_j ascending and the q_e; Q (nb).
 * With ev = q = NULL only start is filled (the size query; Q is not touched).  Every band has at least one entry. */
int spart_srf_support(const double *wl_srf, const double *p_srf, int32_t nsrf, int32_t nb, int32_t *start, int32_t *ev,
                      double *q, double *Q);

/* Bytes of scratch the batched entry points need for B samples (the prelude's per-sample constants, ~0.9 KB per
 * sample, + the band sums of the full-band kernel).  The same buffer may be reused by successive calls
 * on one stream.  spart_smac_batch sizes its workspace with dtype = SPART_F64. */
size_t spart_workspace_bytes(const spart_ctx *ctx, int dtype, int64_t B);

/* Where a spart_run_batch(dtype, B) call that ran the full-band kernel unpruned (prune_unused_bands = 0) leaves its per-chunk
 * band sums in the workspace it was given: *nchunk rows of *row_stride elements starting *offset bytes into the workspace;
 * row c, element b (b < SPART_NWL + 1, b = SPART_NWL the thermal evaluation) = the sum over the samples of chunk c of
 * rso + rdo + rsd + rdd at band b.  With spart_materialize.band_mean the four terms are kept apart instead: four
 * consecutive elements per band (rso, rdo, rsd, rdd), rows of 4 * row_stride.  Elements are of the full-band kernel's type:
 * float for SPART_F32 and with spart_materialize.f32_bands, double otherwise.  The chunks partition the batch in order, so
 * the sum over the rows is the batch total.  A read-only query: it launches nothing and reads no device memory. */
int spart_workspace_bandsum(const spart_ctx *ctx, int dtype, int64_t B, size_t *offset, int64_t *nchunk, int *row_stride);

/* PROSPECT_5D (prospect_5d.py:117-246).  leaf[9] = Cab, Cdm, Cw, Cs, Cca, Cant, N, PROT, CBC.
 * Outputs (B,2001): refl, tran, kChlrel (any may be NULL). */
int spart_prospect_batch(spart_ctx *ctx, int dtype, int64_t B, const double *const leaf[9], void *refl, void *tran,
                         void *kchl, void *workspace, size_t workspace_bytes, void *stream);

/* BSM + soilwat (bsm.py:17-128).  soil[6] = B, lat, lon, SMp, SMC, film.
 * rdry_in: optional (B,2001) user dry spectra in `dtype` (the rdry_set branch, bsm.py:42-43).
 * Outputs (B,2001): refl (wet), refl_dry. */
int spart_bsm_batch(spart_ctx *ctx, int dtype, int64_t B, const double *const soil[6], const void *rdry_in,
                    void *refl, void *refl_dry, void *workspace, size_t workspace_bytes, void *stream);

/* calculate_leafangles (sailh.py:351-398): lidf (B,13) float64. */
int spart_lidf_batch(spart_ctx *ctx, int64_t B, const double *LIDFa, const double *LIDFb, double *lidf, void *stream);

/* SAILH (sailh.py:14-237).  rho, tau, rs: (B,2162) in `dtype`; canopy[4] = LAI, LIDFa, LIDFb, q;
 * angles[3] = sol, obs, rel (degrees).  out4 = rso, rdo, rsd, rdd, each (B,2162).
 * lidf_in, nlayers: the two attributes SAILH reads from the canopy OBJECT (sailh.py:48, 51), with the meaning of the
 * spart_materialize members of the same names: lidf_in optional (B,13) float64 (NULL: from LIDFa / LIDFb; given: canopy[1],
 * canopy[2] may be NULL), nlayers 0 = 60. */
int spart_sailh_batch(spart_ctx *ctx, int dtype, int64_t B, const void *rho, const void *tau, const void *rs,
                      const double *const canopy[4], const double *const angles[3], const double *lidf_in, int32_t nlayers,
                      void *const out4[4], void *workspace, size_t workspace_bytes, void *stream);

/* SMAC (smac.py:14-213).  angles[3]; atm[4] = aot550, uo3, uh2o, Pa.  out9 (B,nb) float64 in the
 * AtmosphericOptics order Ta_s, Ta_o, Tg, Ra_dd, Ra_so, Ta_ss, Ta_sd, Ta_oo, Ta_do (smac.py:209-211). */
int spart_smac_batch(spart_ctx *ctx, int64_t B, const double *const angles[3], const double *const atm[4],
                     double *const out9[9], void *workspace, size_t workspace_bytes, void *stream);

/* SPART(...).run() for a fresh object per sample (SPART.py:162-269).
 * params[27]: Cab Cdm Cw Cs Cca Cant N PROT CBC | B lat lon SMp SMC film | LAI LIDFa LIDFb q |
 *             tts tto psi | aot550 uo3 uh2o Pa | DOY          (each (B,) float64)
 * rho_thermal / tau_thermal: optional (B,) float64 (LeafBiology defaults 0.01 when NULL).
 * Outputs (B,nb) in `dtype`. */
int spart_run_batch(spart_ctx *ctx, int dtype, int64_t B, const double *const params[SPART_NPARAM],
                    const double *rho_thermal, const double *tau_thermal, void *R_TOC, void *R_TOA, void *L_TOA,
                    const spart_materialize *opt, void *workspace, size_t workspace_bytes, void *stream);

/* LUT inversion (the use LUTs are generated for.  The only nearest-index search in the reference is
 * an exact np.argmin with first-index ties, SPART.py:381-387 -- the behaviour kept here):
 * for each of M observed sensor spectra obs (M,nb) find THE row of lut (B,nb) that minimises
 *     c(b, m) = sum_j w_j (lut[b,j] - obs[m,j])^2      (weights (nb,) optional, NULL = 1; expected >= 0)
 * where c is evaluated in `dtype` as  c = 0; for j ascending: d = lut[b,j] - obs[m,j]; c = c + (w_j * d) * d  with every
 * operation rounded to `dtype` and no fused multiply-add.  best_idx (M,) int64 = the LOWEST row index attaining the minimum
 * of that c (bit-exact: the same answer as a brute-force loop, in both dtypes, for any nb), best_cost (M,) = that minimum
 * (divide by nb and take the root for an RMSE).  Rows or observations whose cost is not finite -- NaN, +inf, or -inf (negative
 * weights with overflowing products) -- never win (-1 / +inf when no row has a finite cost); so does a LUT row that holds a
 * non-finite value or whose centred weighted norm sum_j |w_j| (lut[b,j] - centre_j)^2 overflows `dtype` (values near the
 * largest finite number), even if its cost against a particular observation would be finite -- whichever path of the search
 * decides the observation, the brute force included.  A row is judged on its OWN entries: the centres are column means over
 * the entries of magnitude <= 2^62 (SPART_F32) / 2^510 (SPART_F64), a quarter of the square root of the largest number.  A fill
 * value such as FLT_MAX, or an entry of a row that blew up but stayed finite, is thus left out of the centres; the row that holds
 * it is ineligible if its own norm overflows, and every other row's verdict and answer are what they are without it.
 * How: a GEMM with K = nb + 1 on the matrix cores -- exact-f32 v_mfma_f32_32x32x2_f32 for SPART_F32,
 * v_mfma_f64_16x16x4_f64 for SPART_F64 -- over the CENTRED LUT (per-band mean removed) ranks the tiles of 32 / 16 LUT rows by
 * |x'|^2 - 2 x'.y'; every tile whose minimum lies within a proven rounding bound of the best one is then evaluated row by
 * row with c itself, and an observation for which the scan may have missed such a tile is re-done by a brute-force kernel
 * (csrc/spart_lut.h derives the bound).  The data only decide how much of that extra work there is, never the result.
 * All pointers are device memory in `dtype`; nb <= 31; B, M <= 2e9. */
size_t spart_lut_workspace_bytes(int dtype, int64_t B, int nb, int64_t M);
int spart_lut_nearest(spart_ctx *ctx, int dtype, int64_t B, int nb, const void *lut, int64_t M, const void *obs,
                      const void *weights, int64_t *best_idx, void *best_cost, void *workspace, size_t workspace_bytes,
                      void *stream);
/* Diagnostics of the LAST spart_lut_nearest call that used `workspace` (same dtype, B, nb, M): the number of observations
 * that took the brute-force path and Nmax = max_b sum_j |w_j| (lut[b,j] - centre_j)^2, the scale of the rounding bound.
 * Synchronises the device (a blocking copy of 16 bytes).  No reference counterpart. */
int spart_lut_stats(spart_ctx *ctx, int dtype, int64_t B, int nb, int64_t M, const void *workspace, int64_t *n_brute_force,
                    double *nmax);

/* The k nearest LUT rows (the usual inversion of an ill-posed LUT: the mean / median / spread of the k best rows; no reference
 * counterpart).  For each observation m: the k rows with the smallest cost c(b, m) -- the SAME c as spart_lut_nearest, evaluated
 * the same way -- ordered by (cost ascending, row index ascending); exactly np.argsort(c, kind="stable")[:k] after non-finite
 * costs are set to +inf.  Rows whose cost is not finite never appear, under spart_lut_nearest's rules (NaN rows, an overflowing
 * centred norm, -inf); when fewer than k rows qualify the tail is (-1, +inf).  idx (M,k) int64 and cost (M,k) in `dtype`,
 * row-major; entry [m,0] equals spart_lut_nearest's answer bit for bit.  1 <= k <= 256 (SPART_ERR_INVALID otherwise);
 * weights, nb <= 31 and the size limits as for spart_lut_nearest.
 * How (csrc/spart_lut.h derives it): the k = 1 GEMM scan on the matrix cores gives, per observation, k filter values of
 * distinct rows and so a proven threshold; a second GEMM pass lists every tile with a filter value under it; one wave per
 * observation evaluates their rows with c itself and keeps the k best; an observation the filter cannot settle is re-done by
 * a brute-force kernel.  Observations are processed in chunks of 65 536, so the workspace grows with M only by 4 bytes per
 * observation beyond the first chunk. */
size_t spart_lut_topk_workspace_bytes(int dtype, int64_t B, int nb, int64_t M, int k);
int spart_lut_topk(spart_ctx *ctx, int dtype, int64_t B, int nb, const void *lut, int64_t M, const void *obs,
                   const void *weights, int k, int64_t *idx, void *cost, void *workspace, size_t workspace_bytes, void *stream);
/* Diagnostics of the LAST spart_lut_topk call that used `workspace` (same dtype, B, nb, M, k): observations that took the
 * brute-force path, candidate tiles (of 32 rows for SPART_F32, 16 for SPART_F64) summed over the observations and their maximum
 * per observation, and Nmax.  Synchronises the device. */
int spart_lut_topk_stats(spart_ctx *ctx, int dtype, int64_t B, int nb, int64_t M, int k, const void *workspace,
                         int64_t *n_brute_force, int64_t *n_candidates, int64_t *max_candidates, double *nmax);

/* The k nearest LUT rows for ANY 1 <= nb <= SPART_NWLS (hyperspectral sensors): word for word spart_lut_topk's semantics -- the
 * same cost c, evaluated the same way, the same (cost, row) order, the same rules for non-finite rows, observations and norms,
 * (-1, +inf) padding, 1 <= k <= 256, B and M <= 2e9 -- so for nb <= 31 its output equals spart_lut_topk's bit for bit, and
 * column 0 is the exact nearest row (k = 1: spart_lut_nearest's answer).  An nb outside 1..SPART_NWLS is a bad size
 * (SPART_ERR_INVALID).
 * How (csrc/spart_lut.h, "wide top-k", derives the bound): the same filter-then-exact structure with K streamed instead of
 * held in registers -- a norm pass over the LUT (no copy of it: the workspace grows with B and with M nb, never with B nb),
 * a GEMM scan on the matrix cores that stages LUT rows and pre-scaled observations through LDS in chunks of 32 bands, a
 * collecting second GEMM pass, one wave per observation evaluating the candidate rows with c itself, and a brute force for
 * the observations the filter cannot settle.  Observations go in chunks of 16 384. */
size_t spart_lut_topk_wide_workspace_bytes(int dtype, int64_t B, int nb, int64_t M, int k);
int spart_lut_topk_wide(spart_ctx *ctx, int dtype, int64_t B, int nb, const void *lut, int64_t M, const void *obs,
                        const void *weights, int k, int64_t *idx, void *cost, void *workspace, size_t workspace_bytes,
                        void *stream);
/* Diagnostics of the LAST spart_lut_topk_wide call that used `workspace` (same dtype, B, nb, M, k), as spart_lut_topk_stats:
 * brute-forced observations, candidate tiles (32 rows for SPART_F32, 16 for SPART_F64; sum and maximum) and Nmax. */
int spart_lut_topk_wide_stats(spart_ctx *ctx, int dtype, int64_t B, int nb, int64_t M, int k, const void *workspace,
                              int64_t *n_brute_force, int64_t *n_candidates, int64_t *max_candidates, double *nmax);

/* The k nearest LUT rows with ONE WEIGHT ROW PER OBSERVATION (per-pixel noise and per-pixel band masks; no reference
 * counterpart).  weights (M, nb) in `dtype`, device memory, required (NULL: SPART_ERR_INVALID).  For each observation m the
 * cost of row b is, evaluated in `dtype` with every operation rounded and no FMA,
 *     c = 0;  for j = 0 .. nb-1:  if (w[m,j] == 0) continue;  d = lut[b,j] - obs[m,j];  c = c + (w[m,j] * d) * d
 * -- spart_lut_topk_wide's cost plus one rule: a band of weight exactly zero is skipped, so obs[m,j] may be NaN or inf there
 * (the mask).  Rows are ordered by (cost, row), i.e. np.argsort(c, kind="stable")[:k] after non-finite costs are set to +inf;
 * the tail is padded with (-1, +inf); 1 <= k <= 256, 1 <= nb <= SPART_NWLS, B and M <= 2e9 (SPART_ERR_INVALID otherwise).
 *   Rows: a row with a non-finite entry never appears, nor one whose UNWEIGHTED centred norm sum_j (lut[b,j] - centre_j)^2
 *   overflows; row acceptance does not depend on the observation.
 *   Observations: one with a negative, NaN or infinite weight, or a non-finite value in a band of non-zero weight, matches
 *   no row: its whole output row is (-1, +inf).  All weights zero: every accepted row costs 0, the first k accepted rows.
 * So with every weight row equal to w, finite observations and no norm near overflow the result is spart_lut_topk_wide(w)'s
 * bit for bit, and zero weights on a band set S give the answer of the LUT and observation with the columns of S removed.
 * How (csrc/spart_lut.h, "per-observation weights", derives the bound): the wide pipeline with the filter
 * sum_j w_mj x'_bj^2 - 2 sum_j w_mj y'_mj x'_bj as one GEMM of K = 2 nb on the matrix cores; observations go in chunks of at
 * most 16 384 (fewer above ~1000 bands in float64: the operand rows stay within 256 MiB). */
size_t spart_lut_topk_obs_weights_workspace_bytes(int dtype, int64_t B, int nb, int64_t M, int k);
int spart_lut_topk_obs_weights(spart_ctx *ctx, int dtype, int64_t B, int nb, const void *lut, int64_t M, const void *obs,
                               const void *weights, int k, int64_t *idx, void *cost, void *workspace, size_t workspace_bytes,
                               void *stream);
/* Diagnostics of the LAST spart_lut_topk_obs_weights call that used `workspace` (same dtype, B, nb, M, k): brute-forced
 * observations, candidate tiles (32 rows for SPART_F32, 16 for SPART_F64; sum and maximum) and the largest
 * Nbound_m = sum_j w[m,j] max_b (lut[b,j] - centre_j)^2, the scale of the rounding bound. */
int spart_lut_topk_obs_weights_stats(spart_ctx *ctx, int dtype, int64_t B, int nb, int64_t M, int k, const void *workspace,
                                     int64_t *n_brute_force, int64_t *n_candidates, int64_t *max_candidates, double *nbound);

/* The likelihood-weighted (Bayesian / GLUE) LUT estimate: what the LUT AS A WHOLE says about an observation given its noise
 * (no reference counterpart).  Every row b within `cut` of the best one gets the weight exp(-chi^2_b / 2); the outputs are the
 * weighted mean and spread of the parameter rows and the effective sample size, the one number that tells whether the LUT is
 * dense enough for the noise level.  lut (B, nb), obs and weights (M, nb) in `dtype`; weights is required; params (B, P)
 * float64 row-major; all device memory.  T is the dtype.
 * Definition, per observation m.  The cost c_T(b, m), the row acceptance rule and the observation validity rule are
 * spart_lut_topk_obs_weights', word for word: the cost is evaluated in T with every operation rounded and no FMA, a band of
 * weight exactly zero is skipped (obs may be NaN or inf there), a row with a non-finite entry or an overflowing unweighted
 * centred norm is never accepted, and an observation with a negative, NaN or infinite weight, or a non-finite value in a band of
 * non-zero weight, is invalid.
 *   E          the accepted rows with a finite c_T.  If the observation is invalid or E is empty: count 0, best_idx -1,
 *              best_cost +inf, sum_w 0, ess / mean / std NaN.
 *   c*         the minimum of c_T over E; best_idx the lowest row attaining it.  best_idx and best_cost equal
 *              spart_lut_topk_obs_weights(k = 1) bit for bit.
 *   e_b        (double)c_T(b) - (double)c*
 *   S          {b in E : e_b <= cut}, taken in ascending row order; count = |S|
 *   omega_b    exp(-(e_b / (2 tau))) in float64, tau the temperature; 2 tau is formed first, the division is IEEE, the
 *              exponential is the library's (relative error <= 3e-16; exactly 1 at e_b = 0)
 *   sums       float64, sequential over S ascending from 0, no FMA contraction:
 *              sum_w  = sum omega_b
 *              s2     = sum omega_b omega_b,        ess = (sum_w * sum_w) / s2
 *              mean_p = (sum (omega_b x_bp)) / sum_w,               x_bp = params[b, p]
 *              var_p  = (sum ((omega_b d) d)) / sum_w with d = x_bp - mean_p,     std_p = sqrt(var_p)
 * Consequences:
 *   - cut = 0 and a unique minimum: count = 1, ess = 1, std = 0 and mean = params[best_idx] exactly.
 *   - all weights of an observation zero and cut >= 0: S is every accepted row and omega = 1; mean and std are then
 *     spart_lut_summarise's sums over all accepted rows in order.
 *   - the result is the same bit for bit with brute_force 0 or 1, whatever else is in the batch, and whichever chunk the
 *     observation falls in.
 * Refused before anything is launched or written, SPART_ERR_INVALID: a dtype outside 0 / 1; nb outside 1 ... SPART_NWLS; P
 * outside 1 ... 64; B or M < 0 or > 2e9; a NULL opt or out; a NaN or negative cut; a negative, NaN or infinite temperature;
 * brute_force outside 0 / 1; with M > 0 all seven outputs NULL (the outputs of an empty batch have no address); with M > 0
 * and B > 0 a NULL lut, params, obs or weights.
 * SPART_ERR_WORKSPACE as for the searches.  M = 0 launches nothing; B = 0 with M > 0 launches no search and writes the
 * empty-observation outputs (no workspace needed).  spart_lut_bayes_workspace_bytes is 0 exactly for the sizes the call
 * refuses or has no search for (B = 0, M = 0); past the first chunk of observations it grows by 4 bytes per observation (the
 * flag list), like the searches'.
 * How (csrc/spart_lut.h, "likelihood-weighted posterior", derives the threshold): the per-observation-weights filter on the
 * matrix cores with the radius threshold U + cut + Delta(cut) in place of the top-k one, at most 1088 candidate tiles per
 * observation; one wave per observation then sorts its tiles and runs three passes over their rows (minimum; weights and
 * first moments; second moments).  An observation whose candidate list overflows, whose threshold is not finite (cut = +inf),
 * or any observation under brute_force = 1, takes the same three passes over every row of the LUT. */
typedef struct spart_lut_bayes_opt {
  double cut;          /* >= 0 or +inf: rows with e_b <= cut take part */
  double temperature;  /* 0 = 1.0; else finite > 0 */
  int32_t brute_force; /* 0 auto; 1: every observation by the brute-force kernel (same result bit for bit) */
} spart_lut_bayes_opt;
typedef struct spart_lut_bayes_out { /* device memory, each may be NULL, not all */
  double *mean, *std;                /* (M, P) */
  double *sum_w, *ess;               /* (M,)   */
  int64_t *count, *best_idx;         /* (M,)   */
  void *best_cost;                   /* (M,) in dtype */
} spart_lut_bayes_out;
size_t spart_lut_bayes_workspace_bytes(int dtype, int64_t B, int nb, int64_t M);
int spart_lut_bayes(spart_ctx *ctx, int dtype, int64_t B, int nb, const void *lut, int P, const double *params, int64_t M,
                    const void *obs, const void *weights, const spart_lut_bayes_opt *opt, const spart_lut_bayes_out *out,
                    void *workspace, size_t workspace_bytes, void *stream);
/* Diagnostics of the LAST spart_lut_bayes call that used `workspace` (same dtype, B, nb, M), as
 * spart_lut_topk_obs_weights_stats: brute-forced observations, candidate tiles (sum and maximum) and the largest Nbound_m. */
int spart_lut_bayes_stats(spart_ctx *ctx, int dtype, int64_t B, int nb, int64_t M, const void *workspace, int64_t *n_brute_force,
                          int64_t *n_candidates, int64_t *max_candidates, double *nbound);

/* spart_lut_bayes with weighted quantiles: a median and a credible interval of every parameter over the same posterior, which
 * is rarely symmetric (LAI saturates, Cab and Cw pile up at 0, a sparse LUT gives two clusters).  Every argument and every
 * output of spart_lut_bayes keeps its meaning, and the seven base outputs are spart_lut_bayes' bit for bit; quant (M, P, nq)
 * float64 row-major, device memory, is new.  levels is a HOST array of nq levels, read before the call returns.
 * Definition.  E, c*, e_b, S (ascending row order), omega_b and sum_w are spart_lut_bayes', word for word, and so are the row
 * rule, the observation rule and the mask rule.  For observation m, parameter p and level q_i (0 <= q_i <= 1), with
 * x_b = params[b, p] for b in S:
 *   target_i   q_i * sum_w, one float64 multiplication
 *   F_p(v)     the float64 sum of omega_b over the rows b of S with x_b <= v: sequential from 0 in ascending row order, no
 *              FMA; a row that does not qualify adds nothing.  It is the ordered sum that gives sum_w, restricted to a subset.
 *   quant[m, p, i]   the smallest value v among {x_b : b in S} with F_p(v) >= target_i: the inverted-CDF quantile, always a
 *              value of the parameter table, never interpolated.  Of values that compare equal (-0.0 and 0.0) the one in the
 *              lowest row is returned.
 *   NaN        if any x_b over S is NaN, all nq quantiles of that (m, p) are NaN (the rule of spart_lut_summarise's median);
 *              +inf and -inf are ordinary ordered values.  An empty E or an invalid observation: NaN beside spart_lut_bayes'
 *              empty outputs.
 * Two facts the definition leans on:
 *   - F_p is non-decreasing in v: an ordered sum of non-negative terms over a larger subset is never smaller, because every
 *     addition is rounded monotonically.  So the smallest qualifying v is well defined and a bisection finds it.
 *   - if no x is NaN, F_p(max) is sum_w bit for bit (the same additions), and q_i * sum_w <= sum_w: q = 1 gives the maximum
 *     over S and q = 0 the minimum.
 * Consequences:
 *   - cut = 0 and a unique minimum: every quantile is params[best_idx] exactly.
 *   - all weights of an observation zero: omega = 1 and every sum an exact integer, so for dyadic q the result is
 *     sort(x)[max(ceil(q n) - 1, 0)] exactly.  q = 0.5 is therefore the LOWER median, not spart_lut_summarise's averaged one.
 *   - quantiles are non-decreasing in q; levels need not be sorted or distinct, and a level's result does not depend on the
 *     others.
 *   - the same bits with brute_force 0 or 1, in any batch and in any chunk.
 * Refused as spart_lut_bayes refuses, in its order; behind the NULL check of opt and out, SPART_ERR_INVALID for nq outside
 * 1 ... 8, a NULL levels, and a level that is NaN or outside [0, 1] (the message names the first such index).  "Every output
 * is NULL" counts quant as an eighth output; quant == NULL with another output given is accepted and the call is then
 * spart_lut_bayes.  M = 0 launches nothing; B = 0 with M > 0 writes NaN to quant beside the empty outputs.  The workspace is
 * spart_lut_bayes_workspace_bytes', and spart_lut_bayes_stats reads it afterwards as before: the stats of a quantile call equal
 * those of the plain call on the same inputs.
 * How (csrc/spart_lut.h, "weighted quantiles of the posterior"): a second one-wave-per-observation kernel behind each
 * spart_lut_bayes kernel reads the same candidate lists, lane = parameter, and bisects every level of every parameter at once
 * on the order-preserving integer image of the doubles, one pass over S per step with the interval ends snapped to data values:
 * about log2(count) passes, never more than 64. */
typedef struct spart_lut_bayes_q_opt {
  spart_lut_bayes_opt base;
  int32_t nq;           /* 1 ... 8 */
  const double *levels; /* HOST (nq,), each in [0, 1] */
} spart_lut_bayes_q_opt;
typedef struct spart_lut_bayes_q_out {
  spart_lut_bayes_out base;
  double *quant; /* (M, P, nq) row-major, device; may be NULL */
} spart_lut_bayes_q_out;
int spart_lut_bayes_quantiles(spart_ctx *ctx, int dtype, int64_t B, int nb, const void *lut, int P, const double *params, int64_t M,
                              const void *obs, const void *weights, const spart_lut_bayes_q_opt *opt,
                              const spart_lut_bayes_q_out *out, void *workspace, size_t workspace_bytes, void *stream);

/* Parameter summaries of the rows a top-k search selected (what a LUT retrieval reports: maps of LAI, Cab, ... with a spread;
 * no reference counterpart).  params (B, P) float64 row-major, the LUT's parameter table; idx (M, k) int64, the output of any
 * of the three top-k searches; mean / median / std (M, P) float64 and count (M,) int32, any of which may be NULL (not all
 * four).  All device memory.  1 <= P <= 64, 1 <= k <= 256, B and M <= 2e9 (SPART_ERR_INVALID otherwise); M = 0 launches
 * nothing; no workspace; one kernel launch on `stream`.
 * Definition.  For observation m let j_1 < j_2 < ... < j_n be the places with 0 <= idx[m, j] < B, in place order.  Every other
 * value of idx (the -1 padding of the searches, or anything out of range) is skipped: the kernel never forms an address from
 * an index it has not range-checked.  With x_i = params[idx[m, j_i], p], all in float64, no FMA contraction:
 *   count[m]     = n
 *   mean[m, p]   = (((x_1 + x_2) + x_3) + ... + x_n) / n
 *   std[m, p]    = sqrt((((x_1 - mean)^2 + (x_2 - mean)^2) + ...) / n)      (ddof = 0, two passes, the sum in place order)
 *   median[m, p] = NaN if any x_i is NaN; else with s the ascending sort of the x_i: s[(n-1)/2] for odd n and
 *                  (s[n/2 - 1] + s[n/2]) / 2 for even n
 *   n = 0: all three are NaN.
 * These are numpy's mean / median / std(axis=1) of the gathered block with the order of summation pinned, so that the result
 * is one defined number.  Duplicated rows in idx[m] count as often as they appear.  NaN parameter VALUES propagate (numpy's
 * nan* forms, which a host summary may use for padded observations, drop them; LUT parameter tables hold no NaN).
 * How (csrc/spart_lut.h, "parameter summaries"): lane = parameter, 64 / P observations per wave for k <= 64; each place is one
 * coalesced read of a P * 8-byte row; the values wait in LDS, one column per lane, for the second pass of std and for the
 * median, which is selected by rank counting. */
int spart_lut_summarise(spart_ctx *ctx, int64_t B, int P, const double *params, int64_t M, int k, const int64_t *idx,
                        double *mean, double *median, double *std, int32_t *count, void *stream);

/* Bounded Levenberg-Marquardt refinement of F of the 27 parameters per observation around the float64 column path (what a
 * LUT inversion is followed by: a local least-squares fit of the forward model from the best row, the other parameters held
 * fixed; no reference counterpart).  One device-resident call: per iteration ONE forward evaluation of (F + 1) rows per
 * observation -- the trial point and F one-sided finite-difference neighbours, by spart_run_batch's own float64 kernels with
 * prune_unused_bands = 1, thermal inputs at their defaults, no rdry_in / lidf_in -- and one step kernel (cost, accept / reject,
 * normal equations, damped solve, bounds).  Everything is queued on `stream`; nothing synchronises.
 *   base[27]  the start rows, each (M,) float64 device memory (spart_run_batch's params order)
 *   free_cols HOST (F,): the distinct columns 0 ... 26 that are fitted, 1 <= F <= 16;  lo, hi HOST (F,): finite, lo < hi
 *   obs (M, nb), weights NULL / (nb,) / (M, nb) (opt->weights_per_obs = 1): device memory, float64.  A weight of exactly 0
 *             skips its band and obs may be NaN there (the mask rule of spart_lut_topk_obs_weights)
 *   opt->prior_mean, opt->prior_weight  both NULL (no prior), or a Gaussian prior on the free parameters (optimal estimation):
 *             mu_f and p_f = 1 / sigma_f^2, (F,) or (M, F) row-major (opt->prior_per_obs = 1), device memory, float64.  A weight
 *             of exactly 0 puts no prior on that parameter and mu_f may be NaN there
 *   x (M, F), cost (M,): required.  cost0 (M,), std (M, F), n_accept (M,) int32, y (M, nb): each may be NULL
 * Definition (tools/refine_defined.py is the same text in numpy; float64, no FMA contraction, IEEE division and sqrt; every
 * sum and solve in one order, so the result is one defined number whatever the batch):
 *   start   x = base[free] clipped (t = v; if t < lo: t = lo; if t > hi: t = hi), c = +inf, lambda = lambda0, trial t = x,
 *           h_f = rel_step (hi_f - lo_f)
 *   for it = 0 ... n_iter (n_iter + 1 forward calls; call 0 evaluates the start):
 *     rows    p_0 = base with the free columns set to t; p_f = p_0 with column free[f-1] set to t_f + s_f h_f, s_f = +1 if
 *             t_f + h_f <= hi_f else -1;  Y_0 ... Y_F = the chosen sensor column of the rows
 *     cost    c_t = 0; for j ascending: w_j == 0 skips the band, else d_j = Y_0j - obs_j, c_t = c_t + (w_j d_j) d_j;
 *             then, with a prior, for f ascending: p_f == 0 skips, else e_f = t_f - mu_f, c_t = c_t + (p_f e_f) e_f
 *     decide  accept iff c_t < c (a NaN never is).  If the START is not accepted (cost0 not finite, or any negative / NaN /
 *             infinite band or prior weight) the observation is dead: x = the clipped start, cost = cost0 = c_t, n_accept = -1, std = NaN,
 *             y = Y_0, and nothing about it changes afterwards.
 *             accept: x = t, c = c_t, r_j = d_j, J_jf = (Y_fj - Y_0j) / (s_f h_f), y = Y_0; for it > 0 also
 *             lambda = max(lambda / 10, 1e-12), n_accept += 1.  reject: lambda = min(lambda 10, 1e12).
 *     propose (not after it = n_iter) with bands of weight 0 skipped in every sum:
 *             A_ab = sum_j (w_j J_ja) J_jb for a >= b (the lower triangle; j ascending), g_a = sum_j (w_j J_ja) r_j,
 *             then, with a prior, for a ascending with p_a != 0: A_aa = A_aa + p_a, g_a = g_a + p_a e_a (e of the trial just
 *             accepted); these augmented sums are the state of the accepted point (what a rejection restores),
 *             D_a = A_aa if A_aa > 0 else 1, B = A with B_aa = A_aa + lambda D_a;  B delta = -g by Cholesky B = L L^T in
 *             textbook row order (sums over k ascending), forward and back substitution; a pivot !(s > 0) or a non-finite
 *             delta_f gives delta = 0;  t = clip(x + delta).  A delta of 0 re-evaluates x, is not accepted and raises lambda:
 *             the intended handling of singular systems.  There is no early exit: converged observations keep proposing.
 *   std     from the undamped A of the last accepted point: A = L L^T; for each f solve L z = e_f; var_f = sum_{k >= f} z_k^2
 *           (k ascending), std_f = sqrt(var_f); all NaN when the factorisation fails.  With weights = 1 / sigma^2 this is the
 *           linearised 1-sigma uncertainty of the retrieved parameter; with a prior A is J^T W J + S_a^-1, so std is the
 *           linearised posterior 1-sigma.  cost and cost0 include the prior's term; y, r and J do not know of it.
 * So cost <= cost0, and the state after n_iter = k is a prefix of n_iter = k + 1.
 * Observations go in chunks of (1 << 19) / (F + 1), so the workspace is bounded whatever M is: the parameter table
 * (27, (F + 1) Mc), three column blocks, the optimiser's state and spart_workspace_bytes(SPART_F64, (F + 1) Mc) for
 * Mc = min(M, chunk).  spart_refine_workspace_bytes is 0 for sizes the call refuses; it sizes spart_refine_srf's workspace too.
 * Refused before anything is launched or written: SPART_ERR_INVALID for F outside 1 ... 16, a free column outside 0 ... 26 or a
 * duplicate, lo >= hi or a non-finite bound, n_iter outside 0 ... 100, column outside 0 ... 2, a negative or non-finite rel_step /
 * lambda0, a NULL required pointer, exactly one of prior_mean / prior_weight NULL, prior_per_obs outside 0 / 1, M < 0 or
 * M > 2e9; SPART_ERR_NOSENSOR for a context without sensor; SPART_ERR_WORKSPACE for
 * a workspace that is missing or too small.  M = 0 launches nothing. */
typedef struct spart_refine_opt {
  int32_t column;          /* 0 R_TOC, 1 R_TOA, 2 L_TOA */
  int32_t n_iter;          /* 0 ... 100 */
  int32_t weights_per_obs; /* 0: weights NULL or (nb,); 1: (M, nb) */
  int32_t fast_prelude;    /* as spart_materialize.fast_prelude */
  int32_t nlayers;         /* as spart_materialize.nlayers, 0 = 60 */
  double rel_step;         /* 0 = 1e-3 */
  double lambda0;          /* 0 = 1e-2 */
  int32_t prior_per_obs;        /* 0: prior_mean / prior_weight are (F,); 1: (M, F) row-major */
  const double *prior_mean;     /* device memory, float64; NULL with prior_weight NULL = no prior */
  const double *prior_weight;   /* device memory, float64: 1 / sigma_f^2; exactly 0 = no prior on that parameter */
} spart_refine_opt;
size_t spart_refine_workspace_bytes(const spart_ctx *ctx, int64_t M, int F);
int spart_refine(spart_ctx *ctx, int64_t M, const double *const base[SPART_NPARAM], int F, const int32_t *free_cols /* HOST */,
                 const double *lo, const double *hi /* HOST, (F,) */, const double *obs, const double *weights,
                 const spart_refine_opt *opt, double *x, double *cost, double *cost0, double *std, int32_t *n_accept,
                 double *y, void *workspace, size_t workspace_bytes, void *stream);

/* spart_refine with the SRF-convolved columns as the fitted quantity (what a sensor measures, and what a LUT of *_srf columns
 * stores).  Argument for argument spart_refine's list, and its definition word for word with ONE substitution: Y_0 ... Y_F are
 * the chosen SRF-convolved column of the rows -- spart_materialize.R_TOC_srf, R_TOA_srf or L_TOA_srf for opt->column 0, 1 or
 * 2: bit for bit what spart_run_batch(SPART_F64, prune_unused_bands = 1) returns for those rows, with the thermal inputs at
 * their defaults, no rdry_in / lidf_in, opt->fast_prelude and opt->nlayers honoured -- and y is that column at x.  Start, cost,
 * decision, propose and std rules, prior, dead observations, chunking, refusals and their order, SPART_ERR_NOSENSOR, M = 0 and
 * the stream rule are spart_refine's.  The workspace is spart_refine's too: spart_refine_workspace_bytes serves both calls.
 * As for the *_srf outputs the library does what the sensor tables say (see spart_srf_support): a sensor whose SRF samples
 * are not aligned with the model grid is the caller's business.
 * Cost: an iteration evaluates every entry of the compressed SRF support of every band for (F + 1) rows per observation (968
 * model bands per row for Sentinel-2A) where spart_refine evaluates <= 2 nb; the centre column kernel is not launched. */
int spart_refine_srf(spart_ctx *ctx, int64_t M, const double *const base[SPART_NPARAM], int F, const int32_t *free_cols /* HOST */,
                     const double *lo, const double *hi /* HOST, (F,) */, const double *obs, const double *weights,
                     const spart_refine_opt *opt, double *x, double *cost, double *cost0, double *std, int32_t *n_accept,
                     double *y, void *workspace, size_t workspace_bytes, void *stream);

/* spart_refine for several observations of the SAME surface (the cameras of a multi-angle instrument, a few overpasses, a short
 * time series): per pixel ONE unknown vector is fitted against V observations ("views"), each with its own fixed parameters.
 * The first Fs = opt->n_shared entries of free_cols are SHARED (one value for all views), the other Fl = F - Fs are LOCAL (one
 * value per view): n = Fs + V Fl unknowns per pixel, 1 <= n <= 16.  Unknown a < Fs is shared name a; unknown Fs + v Fl + l is
 * local name Fs + l in view v.  With V = 1 the call is spart_refine (band_model 0) / spart_refine_srf (band_model 1) bit for bit.
 *   base[27]  each (V, M) view-major float64 device memory: element [v M + m] is view v of pixel m.  The entries of a shared
 *             column in views 1 ... V-1 are never read (they may be NaN)
 *   free_cols, lo, hi  HOST (F,): one bound pair per NAME
 *   obs, y    (M, V, nb) row-major;  weights NULL, (nb,) applied to every view, or (M, V, nb) (opt->fit.weights_per_obs = 1)
 *   opt->fit  spart_refine's options; prior_mean / prior_weight are (n,) or (M, n) (prior_per_obs = 1), per unknown
 *   x, std    (M, n);  cost, cost0, n_accept (M,)
 * Definition (tools/refine_views_defined.py is the same text in numpy).  Virtual band u = v nb + j; unknown a is ACTIVE in view
 * v if it is shared or a local of view v.
 *   start   shared z_a = base[free[a]] of view 0, clipped; local z_(v,l) = base[free[Fs + l]] of view v, clipped; h_a =
 *           rel_step (hi - lo) of the name
 *   rows    each iteration and view evaluates F + 1 rows: p_(v,0) = view v's base with the free columns taken from the trial
 *           (the shared values and that view's locals); p_(v,f) = p_(v,0) with column free[f-1] moved by s_a h_a of the unknown
 *           it belongs to, s_a by spart_refine's rule on t_a.  One forward call evaluates V (F + 1) rows per pixel
 *   cost    spart_refine's band loop over u ascending (w_u == 0 skips the band), then the prior over the n unknowns ascending
 *   J       J_ua = (Y_f(a)[v, j] - Y_0[v, j]) / (s_a h_a) where a is active in v; elsewhere the entry is structurally absent.
 *           A_ab (a >= b) and g_a are spart_refine's sums over u ascending restricted to the u where a (and b) are active and
 *           w_u != 0: an absent entry is SKIPPED, never multiplied in, so local pairs of different views are exactly 0 and a NaN
 *           in one view's column cannot leak into another view's unknowns
 *   everything else is spart_refine's text with F read as n: decision, dead observations (a pixel is dead as a whole), lambda
 *   and its clamps, the prior's additions, D, Cholesky and its failure rule, clip, std, no early exit, the prefix property,
 *   cost <= cost0.
 * Consequences: a view whose weights are all zero leaves its locals at their clipped start (delta = 0 exactly); without a prior
 * on those locals the undamped A is singular and the pixel's whole std row is NaN; with a prior weight on them std is finite.
 * Pixels go in chunks of max(1, (1 << 19) / ((F + 1) V)); the workspace is bounded by one chunk like spart_refine's.
 * Refused before anything is launched or written: spart_refine's list in its order, with -- after the NULL check of base,
 * free_cols, lo, hi, opt -- V outside 1 ... 64, n_shared outside 0 ... F, n outside 1 ... 16, band_model outside 0 / 1.
 * spart_views_workspace_bytes is 0 exactly for refused sizes (spart_refine_workspace_bytes stays the one size query of
 * spart_refine and spart_refine_srf: this call has its own, named apart). */
typedef struct spart_refine_views_opt {
  spart_refine_opt fit;    /* column, n_iter, weights_per_obs, fast_prelude, nlayers, rel_step, lambda0, the prior */
  int32_t V;               /* views per pixel, 1 ... 64 */
  int32_t n_shared;        /* Fs: the first Fs entries of free_cols are shared, the other F - Fs local */
  int32_t band_model;      /* 0: centre columns (spart_refine's forward call), 1: SRF columns (spart_refine_srf's) */
} spart_refine_views_opt;
size_t spart_views_workspace_bytes(const spart_ctx *ctx, int64_t M, int V, int F, int n_shared);
int spart_refine_views(spart_ctx *ctx, int64_t M, const double *const base[SPART_NPARAM], int F, const int32_t *free_cols /* HOST */,
                       const double *lo, const double *hi /* HOST, (F,) */, const double *obs, const double *weights,
                       const spart_refine_views_opt *opt, double *x, double *cost, double *cost0, double *std, int32_t *n_accept,
                       double *y, void *workspace, size_t workspace_bytes, void *stream);

/* spart_refine with a LINEAR MIXTURE of V canopies per pixel (crop plus bare soil with the cover fraction as an unknown; a MODIS
 * or OLCI pixel over several land covers): the observed column is y_j = sum_v a_v Y_v[j] over V components, each with its own
 * 27-parameter row.  The first Fs = opt->n_shared entries of free_cols are SHARED by all components (soil brightness, atmosphere),
 * the other Fl = F - Fs are LOCAL to a component, and only where opt->local_active says so (LAI and Cab of the crop, not of the
 * bare-soil component); the fractions a_v are given (a land-cover map) or fitted on the simplex.  The chosen column itself is
 * mixed: for R_TOA / L_TOA that neglects the coupling of neighbouring surfaces through the atmosphere.
 *   base[27]  each (V, M) component-major float64 device memory: element [v M + m] is component v of pixel m.  The entries of a
 *             shared column in components 1 ... V-1 are never read (they may be NaN)
 *   free_cols, lo, hi  HOST (F,): one bound pair per NAME
 *   obs       (M, nb);  weights NULL, (nb,) or (M, nb) (opt->fit.weights_per_obs = 1)
 *   frac      (M, V) device: the given fractions, or the start of the fitted ones (its last column is then never read)
 *   opt->fit  spart_refine's options; prior_mean / prior_weight are (n,) or (M, n) (prior_per_obs = 1), per unknown
 *   out       x, std (M, n); cost, cost0, n_accept (M,); y (M, nb) the mixed column at x; frac (M, V) all V fractions at x;
 *             y_comp (M, V, nb) the components' own columns at x.  x and cost are required, every other may be NULL
 * Definition (tools/refine_mix_defined.py is the same text in numpy; float64, no FMA contraction, every sum in one order).
 *   unknowns  in this order: the Fs shared names; the ACTIVE locals, v ascending and within a component l ascending
 *             (local_active is (V, Fl), NULL = all active; an inactive local of a component stays at that component's base value
 *             and is no unknown); with fit_fractions q_0 ... q_{V-2}.  nm counts the model unknowns, n = nm + (V - 1 if
 *             fit_fractions else 0), 1 <= n <= 16, 1 <= V <= 8.  Bounds and step of a model unknown are those of its name; a
 *             fraction unknown has the box [frac_lo, frac_hi] and no step
 *   start     shared: component 0's base; local: its own component's base; q_v: frac[m, v]; everything clipped
 *   rows      a trial evaluates V (F + 1) rows per pixel exactly as spart_refine_views does: block f + 1 of component v moves
 *             column free[f] by s_a h_a of the unknown it belongs to; where that local is inactive in v the block is the unmoved
 *             trial row, evaluated and never read
 *   fractions fitted: s = 0; for v < V - 1 ascending a_v = t[nm + v], s = s + a_v; a_{V-1} = 1 - s.  The trial is FEASIBLE iff
 *             a_{V-1} >= 0 (a NaN is not).  Given: a_v = frac[m, v] as it is, no sum rule; a negative, NaN or infinite entry
 *             makes the pixel dead (the rule of a bad weight)
 *   y         y_j = a_0 Y_(0,0)j; then for v = 1 ... V - 1: y_j = y_j + a_v Y_(v,0)j
 *   cost      spart_refine's band loop on y, then the prior over the n unknowns; after that an infeasible trial's cost is +inf:
 *             an infeasible proposal is rejected and raises lambda, an infeasible start is a dead pixel with cost = cost0 = +inf
 *   J         dense over the nb bands.  Local unknown a of component v, name f: J_ja = a_v ((Y_(v,f+1)j - Y_(v,0)j) / (s_a h_a));
 *             shared unknown: that product for v = 0, then + a_v (...) for v = 1 ... V - 1 ascending; fraction q_v:
 *             J_ja = Y_(v,0)j - Y_(V-1,0)j
 *   everything else is spart_refine's text with F read as n: decision, dead pixels, lambda and its clamps, the sums of A and g,
 *   the prior's additions, D, Cholesky and its failure rule, clip, std, no early exit, the prefix property, cost <= cost0.
 * Consequences: V = 1 is spart_refine (band_model 0) / spart_refine_srf (band_model 1) bit for bit, with or without
 * fit_fractions (1 z and 1 - 0 are exact); the fitted fractions sum to 1 to within one rounding and the last is >= 0 on every
 * live pixel.  Pixels go in chunks of max(1, (1 << 19) / ((F + 1) V)); the workspace is spart_refine_views' layout with this n.
 * Refused before anything is launched or written: spart_refine's list in its order, with -- after the NULL check of base,
 * free_cols, lo, hi, opt, out -- V outside 1 ... 8, n_shared outside 0 ... F, band_model or fit_fractions outside 0 / 1, a
 * local_active entry outside 0 / 1, a local name that is active in no component, n outside 1 ... 16, a bad fraction box, a NULL
 * frac.  M = 0 launches nothing.  spart_mix_workspace_bytes is 0 exactly for refused sizes. */
typedef struct spart_refine_mix_opt {
  spart_refine_opt fit;          /* column, n_iter, weights_per_obs, fast_prelude, nlayers, rel_step, lambda0, the prior */
  int32_t V;                     /* components per pixel, 1 ... 8 */
  int32_t n_shared;              /* Fs: the first Fs entries of free_cols are shared, the other F - Fs local */
  int32_t band_model;            /* 0: centre columns (spart_refine's forward call), 1: SRF columns (spart_refine_srf's) */
  int32_t fit_fractions;         /* 0: frac is given, 1: q_0 ... q_{V-2} are unknowns */
  const int32_t *local_active;   /* HOST (V, Fl) row-major 0 / 1, or NULL = all active */
  double frac_lo, frac_hi;       /* the box of a fitted fraction: both 0 = [0, 1]; else 0 <= lo < hi <= 1 */
} spart_refine_mix_opt;
typedef struct spart_refine_mix_out {
  double *x, *cost, *cost0, *std;
  int32_t *n_accept;
  double *y, *frac, *y_comp;
} spart_refine_mix_out;
size_t spart_mix_workspace_bytes(const spart_ctx *ctx, int64_t M, int V, int F, int n);
int spart_refine_mix(spart_ctx *ctx, int64_t M, const double *const base[SPART_NPARAM], int F, const int32_t *free_cols /* HOST */,
                     const double *lo, const double *hi /* HOST, (F,) */, const double *obs, const double *weights,
                     const double *frac, const spart_refine_mix_opt *opt, const spart_refine_mix_out *out, void *workspace,
                     size_t workspace_bytes, void *stream);

/* Refinement with parameters shared by a TILE of pixels: one atmosphere per window, one leaf-angle parameter per field.  The
 * first Fs = n_shared entries of free_cols are ONE unknown per tile, the other Fl = F - Fs one unknown per pixel; a tile is the
 * contiguous pixels tile_start[t] ... tile_start[t + 1] - 1, at most 4096 of them.  One Levenberg-Marquardt decision is taken
 * per tile on the summed cost; the damped system of a tile is block-arrowhead and is solved by eliminating every pixel's
 * locals.  base, free_cols, lo, hi (per name), obs, weights and opt->fit are spart_refine's; opt->fit.prior_* is the prior of
 * the LOCAL unknowns, (Fl,) or (M, Fl) with prior_per_obs = 1; the prior of the shared ones is shared_prior_*, (Fs,) or (T, Fs).
 * Definition (tools/refine_tiles_defined.py is the same text in numpy; float64, no FMA contraction, IEEE division and sqrt; the
 * per-entry arithmetic is spart_refine's):
 *   order    inside a pixel the unknowns are taken in SOLVE ORDER: every local first (q = b for local name Fs + b), then the
 *            shared (q = Fl + a).  The unknowns of a tile are every live pixel's locals, pixels ascending, then the shared.
 *   start    shared z_a = clip(base[free[a]][tile_start[t]]), the tile's first pixel: the other pixels' entries of a shared
 *            column are never read and may be NaN.  Local l_(m,b) = clip(base[free[Fs + b]][m]).  lambda_t = lambda0.
 *   rows     spart_refine's F + 1 rows per pixel from the tile's trial z and the pixel's trial l; s_f by spart_refine's rule on
 *            the trial value, so a shared name has one sign per tile
 *   c_m      spart_refine's band loop, then the local prior loop, b ascending
 *   dead pixel  decided at it = 0: a negative, NaN or infinite band weight or local prior weight, or c_m not < +inf.
 *            status -1, local = the clipped start, local_std NaN, y = Y_0, pixel_cost = c_m; it takes part in no sum of its
 *            tile for the rest of the call
 *   C        C = 0; for live m ascending: C = C + c_m; then the shared prior loop, a ascending, weight 0 skipped
 *   dead tile   decided at it = 0: no live pixel, a bad shared prior weight, or C not < +inf.  n_accept -1, shared = the clipped
 *            start, cost = cost0 = C, every std of the tile NaN; its live pixels get status 1, y = Y_0, pixel_cost = c_m and
 *            keep the clipped start.  Nothing about the tile changes afterwards
 *   decide   per tile: accept iff C_t < C (a NaN never passes); lambda_t and n_accept move by spart_refine's rules
 *   sums     at an accepted point, per live pixel spart_refine's packed A_m and g_m over the unknowns in solve order (so a
 *            shared row holds (w J_shared) J_local), the local prior added to the local diagonal and to g; per tile, for shared
 *            a >= b: S_ab = 0; for live m ascending: S_ab = S_ab + A_m[a, b]; gs_a likewise; then the shared prior is added to
 *            S_aa and gs_a as spart_refine adds it.  A rejection restores these
 *   propose  D = the diagonal entry if > 0 else 1 (A_m[bb] for a local, S_aa for a shared unknown); B = A + lambda_t D on the
 *            diagonal; B delta = -g by spart_refine's Cholesky text on the tile's matrix in the tile's unknown order, entries
 *            between locals of different pixels skipped: R_m = chol(B_m[local, local]);
 *            W_m[a, j] = (A_m[a, j] - sum_{k < j} W_m[a, k] R_m[j, k]) / R_m[j, j];
 *            Ls from s = B_ab; for live m ascending, k = 0 ... Fl-1: s = s - W_m[a, k] W_m[b, k]; for shared k < b:
 *            s = s - Ls[a, k] Ls[b, k]; the forward substitution in that same order (the locals of m; then the shared with
 *            s = -gs_a; for m ascending, k ascending: s = s - W_m[a, k] d_(m,k); then the shared k < a); the back substitution
 *            of the shared from Fs - 1 down, then each local j from Fl - 1 down with k = j + 1 ... Fl-1 first and the shared a
 *            ascending after.  A pivot !(s > 0) anywhere in the tile, or any non-finite delta, gives delta = 0 for the whole
 *            tile.  t = clip(x + delta).  No early exit
 *   std      from the undamped matrices by spart_refine's std recurrence in the same unknown order: for a shared f, k runs over
 *            the shared unknowns >= f; for a local (m, j), over m's locals >= j and then every shared unknown.  A failed
 *            factorisation makes every std of the tile NaN
 * Consequences.  With every tile one pixel the call is spart_refine (band_model 1: spart_refine_srf) with free_cols = local
 * names then shared names and the two priors concatenated per observation in that order, bit for bit, x / std permuted
 * accordingly (of a dead pixel, which is then a dead tile, cost and cost0 are the TILE's C: no pixel's cost is in it).  A
 * tile's outputs are the same bits whichever other tiles are in the call and whichever chunk it lands in.  A dead pixel in a
 * live tile changes nothing but its own outputs.
 * Pixels go in chunks of whole tiles, greedily: consecutive tiles while the pixel count stays <= 2^19 / (F + 1).  The
 * workspace, spart_tiles_workspace_bytes(ctx, M, F, n_shared), is sized from those three alone, is bounded by one chunk and is
 * 0 exactly for refused sizes.  tile_start is read on the host before the call returns; the call waits for `stream` once per
 * chunk, after it has queued the copy of that chunk's tile map.
 * Refused before anything is launched or written: spart_refine's list in its order (the required outputs -- cost; shared when
 * Fs > 0; local when Fl > 0 -- count as spart_refine's x and cost do), then n_shared outside 0 ... F, then band_model outside
 * 0 / 1, then T < 0 or T = 0 with M > 0, then a bad tile_start (NULL, or the first offending index named), then exactly one
 * shared prior pointer NULL or shared_prior_per_tile outside 0 / 1; SPART_ERR_WORKSPACE, the last of spart_refine's list, comes
 * after these, because n_shared sizes the workspace.  M = 0 launches nothing and, as in spart_refine, returns before them.  Added WITHOUT a new interface number, by spart_refine_srf's rule: two symbols and two structs. */
typedef struct spart_refine_tiles_opt {
  spart_refine_opt fit;    /* column, n_iter, weights_per_obs, fast_prelude, nlayers, rel_step, lambda0; prior_*: the LOCAL prior */
  int32_t n_shared;        /* Fs: the first Fs entries of free_cols are shared by a tile, the other Fl = F - Fs are per pixel */
  int32_t band_model;      /* 0: centre columns (spart_refine's forward call), 1: SRF columns (spart_refine_srf's) */
  int32_t shared_prior_per_tile;                          /* 0: (Fs,), 1: (T, Fs) */
  const double *shared_prior_mean, *shared_prior_weight;  /* device, both NULL or both given */
} spart_refine_tiles_opt;
typedef struct spart_tiles_out {   /* device memory; cost is required, shared when Fs > 0, local when Fl > 0; the rest may be NULL */
  double *shared, *shared_std;     /* (T, Fs) */
  double *local, *local_std;       /* (M, Fl) */
  double *cost, *cost0;            /* (T,) */
  int32_t *n_accept;               /* (T,)  -1: dead tile */
  double *pixel_cost;              /* (M,)  c_m at the accepted point */
  int32_t *status;                 /* (M,)  0 live, -1 dead pixel, 1 live pixel of a dead tile */
  double *y;                       /* (M, nb) */
} spart_tiles_out;
size_t spart_tiles_workspace_bytes(const spart_ctx *ctx, int64_t M, int F, int n_shared);
int spart_refine_tiles(spart_ctx *ctx, int64_t M, const double *const base[SPART_NPARAM], int F, const int32_t *free_cols /* HOST */,
                       const double *lo, const double *hi /* HOST, (F,) per name */, int64_t T, const int64_t *tile_start /* HOST (T+1,) */,
                       const double *obs, const double *weights, const spart_refine_tiles_opt *opt, const spart_tiles_out *out,
                       void *workspace, size_t workspace_bytes, void *stream);

/* Refinement of TIME SERIES of a pixel with a smoothness prior: a season of overpasses in which LAI or Cab move slowly from
 * date to date, leaf angle or soil brightness stay fixed and some dates are cloudy.  A ROW is one date of one pixel and carries
 * its own 27 base parameters (geometry, atmosphere, DOY), obs row and weights, exactly as a pixel of spart_refine_tiles; series
 * s is the contiguous rows series_start[s] ... series_start[s + 1] - 1, at most 256 of them (the std recurrence is quadratic
 * in the length).  The first Fs = n_shared names are one unknown per series and start from the series' first row, the other
 * Fl = F - Fs >= 1 are one unknown per row.  The temporal regulariser (EO-LDAS, the Whittaker smoother) is a first-difference
 * penalty between consecutive rows of a series: the damped system is block-tridiagonal with a border, O(rows) to factorise;
 * the gap under a cloud is filled by its neighbours.  spart_tiles_out is reused with "tile" read as series.
 * Definition (tools/refine_series_defined.py is the same text in numpy): spart_refine_tiles' text with these additions; float64,
 * no FMA contraction, IEEE division and sqrt, every sum in one pinned order.
 *   kappa    for row m with a successor in its series and local b: kappa_(m,b) = smooth[b] * link[m], one multiplication
 *            (link NULL: link[m] = 1).  kappa == 0: that tie is absent.  The link entry of a series' last row is never read
 *   dead     decided at it = 0.  A row is bad by tiles' rule (a bad band weight, a bad local prior weight, c_m not < +inf) or
 *            if a link entry that is read is negative, NaN or infinite.  A series with any bad row, a bad shared prior weight
 *            or C not < +inf is dead AS A WHOLE (a chain cannot lose a link): n_accept -1, shared and local at the clipped
 *            start, cost = cost0 = C, every std NaN, y = Y_0, pixel_cost = c_m; its bad rows get status -1, the others 1.
 *            A row whose weights are all zero is live with c_m = 0: the masked date; obs may be NaN there
 *   C        C = 0; for m ascending: C = C + c_m; then for m ascending over rows with a successor, b ascending, kappa != 0:
 *            e = t_(m+1,b) - t_(m,b) on the trial values, C = C + (kappa e) e; then the shared prior loop as in tiles
 *   sums     at an accepted point each row has tiles' packed A_m, g_m (local prior included), then for local b of row m: if m
 *            has a predecessor with kappa_(m-1,b) != 0: A_m[bb] = A_m[bb] + kappa_(m-1,b), g_(m,b) = g_(m,b) + kappa_(m-1,b)
 *            e_(m-1,b); if m has a successor with kappa_(m,b) != 0: A_m[bb] = A_m[bb] + kappa_(m,b), g_(m,b) = g_(m,b) -
 *            kappa_(m,b) e_(m,b).  The entry between (m+1, b) and (m, b) is -kappa_(m,b).  S, gs are tiles'.  A rejection
 *            restores all of it
 *   propose  D and lambda are tiles', on the augmented diagonal.  B delta = -g by spart_refine's Cholesky text in the unknown
 *            order row 0's locals, row 1's locals, ..., then the shared, over the structurally present entries only: a row's
 *            own local block, the full Fl x Fl block between rows m + 1 and m (present iff some kappa_(m,.) != 0; it starts
 *            from -kappa on its diagonal and 0.0 elsewhere), every shared x local entry, the shared block.  A sum runs over
 *            the k present in both of its rows, ascending in that order; everything else is skipped, never multiplied in as a
 *            zero: X_m[i, j] = (B[(m+1,i),(m,j)] - sum_{k<j} X_m[i,k] R_m[j,k]) / R_m[j,j]; R_(m+1) subtracts X_m's rows
 *            (k = 0 ... Fl-1), then its own k < j; W_(m+1)[a, j] subtracts W_m[a,k] X_m[j,k] (k = 0 ... Fl-1), then its own
 *            k < j; the Schur sums over m then k are tiles'.  Forward and back substitution in the same order (back, local
 *            (m, j): the row's k = j+1 ... Fl-1, the next row's i = 0 ... Fl-1 through X_m[i, j], the shared a ascending).  A
 *            pivot !(s > 0) or a non-finite delta anywhere gives delta = 0 for the series.  t = clip(x + delta).  No early exit
 *   std      from the undamped factors by spart_refine's std recurrence in the same order: for a local (m, j), k runs over m's
 *            locals >= j, then every later row's locals, then the shared (their right-hand sides summed over m then i); for a
 *            shared unknown as in tiles.  A failed factorisation gives NaN for the whole series.  With shared_std and
 *            local_std both NULL none of this is computed
 * Consequences.  With every smooth[b] = 0 (or link all zero) and no bad row the call is spart_refine_tiles on tiles equal to the
 * series, bit for bit in every output; with one-row series it is spart_refine / spart_refine_srf in tiles' permuted form.  A
 * series' bits depend on neither the other series nor the chunk.  cost <= cost0, and n_iter = k is a prefix of k + 1.  With
 * smooth[b] = 0 a masked date's local b stays at its clipped start exactly and, without a prior, the series' std is NaN; with
 * smooth[b] > 0 and link > 0 on at least one side it moves and std is finite.
 * Rows go in tiles' greedy chunks of whole series (one series always fits); spart_series_workspace_bytes(ctx, M, F, n_shared)
 * is 0 exactly for refused sizes (Fl = 0 included).  series_start and smooth are read on the host before the call returns.
 * Refused before anything is launched or written: spart_refine_tiles' list in its order (series_start under the 256-row rule),
 * then Fl = 0 ("nothing to link: use spart_refine_tiles"), then a NULL smooth or an entry of it that is negative, NaN or
 * infinite (the first index named), then SPART_ERR_WORKSPACE.  M = 0 launches nothing.  Second differences, the joint
 * covariance of a series and series of more than 256 rows are out of scope.  Added WITHOUT a new interface number, by
 * spart_refine_srf's rule: two symbols and one struct that embeds spart_refine_tiles_opt unchanged. */
typedef struct spart_refine_series_opt {
  spart_refine_tiles_opt tiles;  /* unchanged: fit (local prior), n_shared, band_model, shared prior (per series) */
  const double *smooth;          /* HOST (Fl,): gamma_b >= 0, finite; one per LOCAL name, in free_cols order */
  const double *link;            /* DEVICE (M,) float64 or NULL (= 1): link[m] scales the tie between rows m and m + 1 */
} spart_refine_series_opt;
size_t spart_series_workspace_bytes(const spart_ctx *ctx, int64_t M, int F, int n_shared);
int spart_refine_series(spart_ctx *ctx, int64_t M, const double *const base[SPART_NPARAM], int F, const int32_t *free_cols /* HOST */,
                        const double *lo, const double *hi /* HOST, (F,) per name */, int64_t S, const int64_t *series_start /* HOST (S+1,) */,
                        const double *obs, const double *weights, const spart_refine_series_opt *opt, const spart_tiles_out *out,
                        void *workspace, size_t workspace_bytes, void *stream);

/* GLOBAL, variance-based sensitivity of a sensor column to the free parameters over their ranges: Sobol' first-order and total
 * indices of every band, with delete-one-block jackknife standard errors -- what says WHICH parameters a retrieval can free.
 * M is the number of SITES: base[p] is (M,) device float64, one fixed row per site (its geometry, atmosphere and everything not
 * freed).  The designs uA, uB (N, F) row-major on the device, in the unit cube, are shared by all sites and used as given: the
 * library holds no random numbers and checks no range; a NaN or out-of-range u gives the x it gives.
 * Definition (tools/sobol_defined.py is the same text in numpy), per site m, float64, every written operation one rounded
 * operation, no FMA contraction, IEEE division and sqrt:
 *   points    xA[n,f] = lo_f + uA[n,f] * (hi_f - lo_f), the difference formed first; xB likewise from uB
 *   rows      A_n is base_m with column free[f] = xA[n,f] for every f; B_n the same with xB; C^f_n = A_n with the one column
 *             free[f] = xB[n,f]: N (F + 2) rows.  yA, yB, yC^f (N, nb) are the chosen column of those rows, bit for bit what
 *             spart_run_batch(SPART_F64, prune_unused_bands = 1) returns for them (thermal inputs at their defaults, no rdry_in /
 *             lidf_in, fast_prelude and nlayers honoured); with band_model 1 the *_srf column instead
 *   shift     c_j = yA[0,j];  a = yA - c,  b = yB - c,  d^f = (yC^f - c) - a.  The estimators are shift-invariant in exact
 *             arithmetic; the shift only keeps E[y^2] - E[y]^2 from cancelling
 *   blocks    block g is samples 64 g ... 64 g + 63.  For each of the Q = 4 + 3 F quantities the 64 per-sample terms t_0 .. t_63
 *             are joined by one fixed tree: for s = 32, 16, 8, 4, 2, 1: t_r = t_r + t_{r+s} for r < s; the result is t_0.
 *             The quantities: sa = a, sb = b, saa = a*a, sbb = b*b, and per f: u_f = b*d^f, t_f = d^f*d^f, e_f = d^f
 *   totals    each quantity summed over the blocks g ascending from 0.0: SA, SB, SAA, SBB, U_f, T_f, D_f
 *   finish    with n = (double)N:  mu = (SA + SB) / (2 n);  m2 = (SAA + SBB) / (2 n);  var = m2 - mu*mu;  mean = c + mu;
 *             S1_f = (U_f / n - mu * (D_f / n)) / var;  ST_f = (T_f / (2 n)) / var  -- Saltelli et al. 2010, Table 2 (b) and (f),
 *             on mean-centred outputs (Sobol' & Levitan 1999).  A zero or non-finite var, or a NaN row, propagates as IEEE
 *             gives: nothing is clamped and nothing is replaced by 0
 *   jackknife with G = N / 64: for each g the finish formulas on X - x_g for every total X (one subtraction each) with
 *             n' = n - 64 give theta_g for each of the 2 F indices;  thetabar = (sum_g theta_g, g ascending from 0.0) / G;
 *             v = 0; for g ascending: e = theta_g - thetabar, v = v + e*e;  se = sqrt((v * (G - 1)) / G)
 * Consequences (a row's column is a pure function of its own 27 parameters).  A site's outputs are the same bits alone or among
 * other sites, in whichever chunk it falls.  Permuting free_cols / lo / hi together with the columns of uA / uB permutes S1, ST
 * and the two se and leaves mean and var unchanged.  With uB == uA every d^f is exactly 0, so S1, ST and both se are 0.  DOY
 * (column 26) as a free parameter with column 0 or 1 gives S1 == ST == 0 for it (only L_TOA reads it) and leaves the other
 * parameters' indices bit-equal to the call without it.
 * Forward rows go in chunks of whole blocks of 64 (F + 2) rows, at most 2^19 rows per chunk, site-major: many small sites
 * share a forward call, a large site runs over several.  spart_sobol_workspace_bytes is 0 exactly for refused sizes; with
 * G = N / 64, bcap = min(M G, 2^19 / (64 (F + 2))) blocks, R = 64 (F + 2) bcap rows and nslot = min(M, bcap / G + 2) it is
 * (each term rounded up to 256 bytes)
 *   8 * 27 R  +  3 * 8 R nb  +  forward scratch of R rows  +  8 nslot nb  +  8 nslot G nb Q:
 * one chunk of forward rows plus the block sums of the sites in flight, constant in M once M G >= 2^19 / (64 (F + 2)).
 * Everything is queued on `stream`; nothing synchronises.  Refused before anything is launched or written: SPART_ERR_INVALID
 * for a NULL context; F outside 1 ... 16; NULL free_cols / lo / hi; column, nlayers; a free column out of range or named
 * twice, bounds not finite lo < hi (spart_refine's checks in its order); then band_model outside 0 / 1; then N not a multiple of
 * 64 or outside 128 ... 2^20; then M < 0 or M > 2e9; then, with M > 0, a NULL opt, out, base or base column (the first named),
 * a NULL uA or uB, or all six outputs NULL.  Then SPART_ERR_NOSENSOR, then (M = 0 launches nothing) SPART_ERR_WORKSPACE.
 * Second-order indices, bootstrap intervals, grouped parameters and designs made on the device are out of scope.  Added WITHOUT
 * a new interface number, by spart_refine_srf's rule: two symbols, two structs. */
typedef struct spart_sobol_opt {
  int32_t column;        /* 0 R_TOC, 1 R_TOA, 2 L_TOA */
  int32_t band_model;    /* 0 centre columns, 1 SRF columns (spart_refine_srf's forward call) */
  int32_t fast_prelude;  /* as spart_materialize */
  int32_t nlayers;       /* as spart_materialize, 0 = 60 */
} spart_sobol_opt;
typedef struct spart_sobol_out {      /* device, float64, each may be NULL, not all */
  double *mean, *var;                 /* (M, nb)    over the 2N rows of A and B, ddof 0 */
  double *S1, *ST;                    /* (M, nb, F) first-order and total index */
  double *S1_se, *ST_se;              /* (M, nb, F) delete-one-block jackknife standard errors */
} spart_sobol_out;
size_t spart_sobol_workspace_bytes(const spart_ctx *ctx, int64_t M, int64_t N, int F);
int spart_sobol(spart_ctx *ctx, int64_t M, const double *const base[SPART_NPARAM], int F,
                const int32_t *free_cols /* HOST */, const double *lo, const double *hi /* HOST (F,) */,
                int64_t N, const double *uA, const double *uB /* DEVICE (N, F) row-major, unit cube */,
                const spart_sobol_opt *opt, const spart_sobol_out *out,
                void *workspace, size_t workspace_bytes, void *stream);

/* The SHAPE of the posterior around a fit, sampled with the forward model itself: the affine-invariant ensemble sampler
 * (Goodman & Weare 2010) in the two-half-ensemble stretch-move form of emcee (Foreman-Mackey et al. 2013), W walkers per
 * observation inside the box lo ... hi, for M observations at once.  It has no proposal scale to tune.  base, free_cols, lo, hi,
 * obs, weights and the prior (opt->prior_*) are spart_refine's, with its mask rule and its weights_per_obs / prior_per_obs
 * forms; the density sampled is exp(-cost / (2 temperature)) on the box, cost being spart_refine's (prior included).
 * The random numbers are made on the device by a counter-based generator and are a pure function of (seed, global observation
 * number, step, walker, draw): the call is one defined result, the same bits in any batch, chunk or launch shape.
 * Definition (tools/sample_defined.py is the same text in numpy), per observation m, float64, every written operation one
 * rounded operation, no FMA contraction:
 *   numbers   Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85); key = (low, high 32
 *             bits of seed); counter = (low 32 bits of g, high 32 bits of g, s mod 2^32, (k << 8) | d) with g = obs_offset + m,
 *             s the absolute step, k the walker, d the draw; output words w0 .. w3.
 *             u53(a, b) = ((a >> 5) * 2^26 + (b >> 6)) * 2^-53: exact, in [0, 1)
 *   start     (s = step0)  x0 = clip(base[free]) by spart_refine's clip; r_f = init_radius[m, f] if given, else
 *             rel_init * (hi_f - lo_f).  Without init: walker k, coordinate f takes the block (s = step0, k, d = f),
 *             u = u53(w0, w1), a_f = max(lo_f, x0_f - r_f), b_f = min(hi_f, x0_f + r_f), x_kf = a_f + u * (b_f - a_f), the
 *             difference formed first; nothing is clipped.  With init: x_k as given.  The costs c_k: the rows are base_m with
 *             the free columns set to x_k; spart_refine's cost, then the prior's term; half 0, then half 1, by a step's path
 *   dead      status -1: a negative, NaN or infinite band or prior weight; a radius not finite and > 0; a given init
 *             coordinate outside [lo, hi] or NaN; a non-finite start cost of any walker.  Every floating output of a dead
 *             observation is NaN and its n_accept is -1; nothing else depends on it
 *   step      for s = step0 + 1 ... step0 + n_steps, and within s for h = 0, 1, the walkers k of half h (h W/2 <= k < (h+1) W/2)
 *             move together against the other half as it stands.  Block d = 0: u1 = u53(w0, w1), partner
 *             j = (1 - h) W/2 + (w2 mod W/2); block d = 1: u2 = u53(w0, w1).  t = (a - 1) * u1 + 1;  z = (t * t) / a;
 *             y_f = x_jf + z * (x_kf - x_jf).  Inside iff lo_f <= y_f <= hi_f for every f (a NaN is outside).  The forward row is
 *             base_m with the free columns at y (for an outside proposal at x_k; the result is then ignored).  c' = cost(y),
 *             prior included;  zp = 1 multiplied by z F - 1 times;  q = zp * exp(-((c' - c_k) / (2 * temperature))).
 *             Accept iff inside and u2 < q (a NaN never accepts): x_k = y, c_k = c', n_accept += 1
 *   best      after the start and after every half-step, for k ascending in that half: c_k < best_cost, strictly, takes the
 *             walker into best_x, best_cost (the first-seen minimum)
 *   kept      step s is kept iff s - step0 > burn and (s - step0 - burn) % thin == 0, as keep number t = 0 ... n_keep - 1,
 *             n_keep = (n_steps - burn) / thin: chain[m, t] and chain_cost[m, t] take the ensemble, and with k ascending
 *             e_f = x_kf - x0_f,  S_f += e_f,  Q_ab += e_a * e_b for a >= b
 *   finish    n = (double)(n_keep W);  mean_f = x0_f + S_f / n;  cov_ab = Q_ab / n - (S_a / n) * (S_b / n), mirrored;
 *             std_f = sqrt(cov_ff);  nothing is clamped.  last, last_cost are the final ensemble
 * exp is the one operation not pinned to the bit (the library's exp_poly, within 3e-16 relative of a correctly rounded exp):
 * a decision whose |u2 - q| / q is below 1e-12 may differ between implementations; the chance is 2e-12 per decision.
 * Consequences.  An observation's outputs are the same bits alone or among others, in whichever chunk it falls: rows [a, b)
 * sampled with obs_offset = a give the rows of the whole call.  A run of n1 + n2 steps, and a run of n1 steps followed by a run
 * of n2 steps with init = last and step0 = n1, give the same last, last_cost and kept states.  With F = 1, zp = 1.
 * Observations go in chunks of Mc = min(M, 2^19 / (W/2)); a chunk runs all its steps before the next starts, 2 (n_steps + 1)
 * forward calls of Mc W/2 rows each, everything queued on `stream`, nothing synchronises.  spart_sample_workspace_bytes is 0
 * exactly for refused sizes; with R = Mc W/2 it is (each term rounded up to 256 bytes)
 *   8 * 27 R  +  3 * 8 R nb  +  forward scratch of R rows  +  the state: 8 Mc (W F + W + 3 F + F (F + 1) / 2 + 2) + 4 Mc
 *   +  8 * 2 R + 4 R + 64 + 88 (the hand-over between the kernels), constant in M once M >= 2^19 / (W/2).
 * Refused before anything is launched or written, SPART_ERR_INVALID: a NULL context; F outside 1 ... 16; NULL free_cols / lo /
 * hi; then spart_refine's checks of the fit in its order (column, nlayers, prior_per_obs, prior_mean without prior_weight or the
 * reverse, a free column out of range or named twice, bounds not finite lo < hi); then band_model outside 0 / 1; W not one of 8,
 * 16, 32, 64 or < 2 F; n_steps outside 1 ... 2^20, burn outside 0 ... n_steps - 1, thin < 1 or n_keep < 1; a not 0 and not
 * finite > 1; temperature not 0 and not finite > 0; rel_init not 0 and not finite > 0; step0 or obs_offset < 0; M < 0 or
 * M > 2e9; then, with M > 0, a NULL opt, out, base or base column (the first named), a NULL obs, weights_per_obs without
 * weights, or all eleven outputs NULL.  Then SPART_ERR_NOSENSOR, then (M = 0 launches nothing) SPART_ERR_WORKSPACE.
 * Other moves, parallel tempering and posterior-predictive spectra are out of scope.  Added WITHOUT a new interface number, by
 * spart_refine_srf's rule: two symbols, two structs. */
typedef struct spart_sample_opt {
  int32_t column;          /* 0 R_TOC, 1 R_TOA, 2 L_TOA */
  int32_t band_model;      /* 0 centre columns, 1 SRF columns (spart_sobol's meaning) */
  int32_t fast_prelude;    /* as spart_materialize */
  int32_t nlayers;         /* as spart_materialize, 0 = 60 */
  int32_t weights_per_obs; /* as spart_refine_opt */
  int32_t prior_per_obs;   /* as spart_refine_opt */
  const double *prior_mean, *prior_weight;  /* as spart_refine_opt: both NULL, or (F,) / (M, F) on the device */
  int32_t W;               /* walkers: 8, 16, 32 or 64, and W >= 2 F */
  int32_t reserved;        /* 0 */
  int64_t n_steps;         /* 1 ... 2^20 */
  int64_t burn;            /* 0 ... n_steps - 1 */
  int64_t thin;            /* >= 1; n_keep = (n_steps - burn) / thin >= 1 */
  double a;                /* stretch scale, 0 = 2.0, else finite and > 1 */
  double temperature;      /* 0 = 1.0, else finite and > 0 (spart_lut_bayes's tau) */
  double rel_init;         /* 0 = 0.01 */
  const double *init_radius; /* NULL, or device (M, F) */
  const double *init;      /* NULL, or device (M, W, F): a given ensemble, for resuming */
  int64_t step0;           /* >= 0: steps already taken */
  int64_t obs_offset;      /* >= 0: global number of observation 0 */
  uint64_t seed;
} spart_sample_opt;
typedef struct spart_sample_out {     /* device, each may be NULL, not all */
  double *mean;                       /* (M, F) */
  double *cov;                        /* (M, F, F) */
  double *std;                        /* (M, F) */
  double *best_x, *best_cost;         /* (M, F), (M,) */
  int64_t *n_accept;                  /* (M,) accepted proposals of all walkers, -1: dead */
  int32_t *status;                    /* (M,) 0, or -1: dead */
  double *chain, *chain_cost;         /* (M, n_keep, W, F), (M, n_keep, W) */
  double *last, *last_cost;           /* (M, W, F), (M, W) */
} spart_sample_out;
size_t spart_sample_workspace_bytes(const spart_ctx *ctx, int64_t M, int F, int W);
int spart_sample(spart_ctx *ctx, int64_t M, const double *const base[SPART_NPARAM], int F,
                 const int32_t *free_cols /* HOST */, const double *lo, const double *hi /* HOST (F,) */,
                 const double *obs, const double *weights, const spart_sample_opt *opt, const spart_sample_out *out,
                 void *workspace, size_t workspace_bytes, void *stream);

/* What spart_refine's optimal-estimation fit knows about a point, kept instead of reduced to std: the Jacobian of the chosen
 * sensor column with respect to the free parameters, the full posterior covariance A^-1 = (J^T W J + S_a^-1)^-1, the averaging
 * kernel A^-1 J^T W J and its trace, the degrees of freedom for signal.  ONE evaluation of the point: the init kernel's table,
 * one forward call of (F + 1) rows per observation, one kernel.  base, free_cols, lo, hi, weights and opt are spart_refine's;
 * obs may be NULL (no measurement: sensitivities and the covariance a measurement WOULD give).  opt->n_iter and opt->lambda0
 * are checked but not used.  band_model 0 evaluates spart_refine's centre columns, 1 spart_refine_srf's SRF columns.
 * Definition per observation (tools/refine_posterior_defined.py is the same text in numpy; float64, no FMA contraction, IEEE
 * division and sqrt):
 *   point   x = clip(base[free]); h_f, s_f (by spart_refine's rule on x_f) and the rows p_0 ... p_F as in spart_refine;
 *           Y_0 ... Y_F = the chosen column of the rows
 *   cost    spart_refine's band loop and prior loop at t = x, same order, same skip rules; with obs == NULL the band loop adds
 *           nothing (c = 0 before the prior's terms).  nband counts w_j != 0
 *   dead    status = -1: a band or prior weight negative, NaN or infinite, or a cost that is not < +inf.  x, y = Y_0, cost and
 *           nband are written; jac, cov, ak, std and dfs are NaN
 *   J       J_jf = (Y_fj - Y_0j) / (s_f h_f) for EVERY band j, bands of weight 0 included
 *   K       the data part alone: K_ab = sum_j (w_j J_ja) J_jb for a >= b, j ascending, w_j == 0 skipped.  A = K; then for a
 *           ascending with p_a != 0: A_aa = A_aa + p_a
 *   factor  A = L L^T by spart_refine's Cholesky; a pivot !(s > 0) gives status = 1: cov, ak, std and dfs are NaN while x, y,
 *           jac, cost and nband stay valid
 *   cov     Z = L^-1, column f by std's recurrence z_k = ((k == f) - sum_{f <= i < k} L_ki z_i) / L_kk (i ascending);
 *           cov_ab for a >= b is v = 0; for k = a ... F-1: v = v + Z_ka Z_kb, copied to (b, a); std_f = sqrt(cov_ff)
 *   ak, dfs K mirrored to full; ak_ab = 0; for c = 0 ... F-1: ak_ab = ak_ab + cov_ac K_cb;  dfs = 0; for a ascending:
 *           dfs = dfs + ak_aa
 * Consequences.  Called on the rows a fit returned -- base with the free columns set to spart_refine's x, the same bounds,
 * weights, prior and options -- std, y and cost equal the fit's bit for bit: the columns are a pure function of a row's own 27
 * parameters, clip(x) = x, and the step signs are those of the accepted trial.  Without a prior ak is the identity up to
 * rounding and dfs = F.  With all band weights zero and a prior, K = 0: ak and dfs are exactly 0 and cov = diag(1 / p) up to
 * rounding.
 * The workspace is spart_refine_workspace_bytes(ctx, M, F); observations go in spart_refine's chunks; jac's offsets are 64-bit.
 * Refused before anything is launched or written: spart_refine's list in its order (obs is not required), out NULL with the
 * other NULL arguments, then band_model outside 0 / 1, then all ten output pointers NULL; SPART_ERR_NOSENSOR and
 * SPART_ERR_WORKSPACE as for spart_refine.  M = 0 launches nothing.  Everything is queued on `stream`; nothing synchronises.
 * Added WITHOUT a new interface number, by spart_refine_srf's rule: one more symbol and one new struct. */
typedef struct spart_posterior_out {   /* device memory; each may be NULL, not all of them */
  double *x;      /* (M, F)      the point: base[free] clipped */
  double *y;      /* (M, nb)     the chosen column at x */
  double *jac;    /* (M, nb, F)  J_jf, row-major, EVERY band (weight-0 bands included) */
  double *cov;    /* (M, F, F)   A^-1, full and exactly symmetric */
  double *ak;     /* (M, F, F)   averaging kernel A^-1 K (not symmetric) */
  double *std;    /* (M, F)      sqrt(cov_ff) */
  double *dfs;    /* (M,)        trace of ak */
  double *cost;   /* (M,)        spart_refine's cost at x, prior term included */
  int32_t *nband; /* (M,)        bands with weight != 0 */
  int32_t *status;/* (M,)        0 ok, 1 A not positive definite, -1 dead */
} spart_posterior_out;
int spart_refine_posterior(spart_ctx *ctx, int64_t M, const double *const base[SPART_NPARAM], int F, const int32_t *free_cols /* HOST */,
                           const double *lo, const double *hi /* HOST, (F,) */, const double *obs /* may be NULL */,
                           const double *weights, const spart_refine_opt *opt, int band_model /* 0 centre, 1 srf */,
                           const spart_posterior_out *out, void *workspace, size_t workspace_bytes, void *stream);

/* Canopy products of a parameter row: what a vegetation product publishes next to LAI (no reference counterpart).  Five
 * numbers per sample, float64, each a deterministic function of the row's leaf, soil and canopy parameters and the sun zenith
 * angle tts.  They do not depend on tto, psi, the atmosphere, DOY or a sensor: a context without a sensor (nb = 0) serves.
 * A LUT carries them as further columns of its parameter table (spart_amd.lut_products), so that the k nearest rows or the
 * posterior weights average the product itself and not the product of the averaged inputs.
 * Definition (tools/products_defined.py is the same text in numpy on the oracle's operations).  For model band i = 0 ... 2000
 * (400 + i nm): rho, tau the PROSPECT leaf, rs the wet BSM soil, tss = exp(-k LAI) (sailh.py:200), rho_dd, tau_dd, tau_sd,
 * rho_sd of sailh.py:205-209, Ea the context's ET irradiance table.
 *     d      = 1 - rs rho_dd
 *     rsd    = rho_sd + (tss + tau_sd) rs tau_dd / d            sailh.py:232, what the library already returns
 *     rdd    = rho_dd + tau_dd rs tau_dd / d                    sailh.py:233
 *     a_s    = 1 - rsd - (1 - rs) (tss + tau_sd) / d            canopy absorptance, direct illumination
 *     a_d    = 1 - rdd - (1 - rs) tau_dd / d                    canopy absorptance, diffuse illumination
 *     fAPAR_bs  = sum_{i=0..300}  Ea_i a_s,i / sum_{i=0..300}  Ea_i       400-700 nm
 *     fAPAR_ws  = the same with a_d
 *     albedo_bs = sum_{i=0..2000} Ea_i rsd_i / sum_{i=0..2000} Ea_i       400-2400 nm
 *     albedo_ws = the same with rdd
 *     fCover    = 1 - exp(-LAI sum_{j=0..12} lidf_j cos(litab_j pi / 180))
 * lidf is what spart_lidf_batch returns (the literal iteration), litab is sailh.py:49; the fCover exponent is the reference's
 * volscatt at tto = 0, where chi_o = cos(theta_l).  The (1 - rs)(.) / d terms are the flux the soil absorbs, so each absorptance
 * is an energy balance on the model's own fluxes.  The thermal evaluation takes no part.  A NaN in a parameter a product reads
 * gives NaN (fCover reads LAI, LIDFa and LIDFb only; the other four read every leaf, soil and canopy parameter but q, and tts).
 * One exception, as everywhere in the library: SMp and SMC enter through the test mu > 0 (bsm.py:101), which a NaN fails, so a
 * NaN there is a dry soil.
 * Blue-sky mixing, (1 - f_dif) bs + f_dif ws, is the caller's business.
 * The model as it is.  sailh.py:189 has denom = 1 - rinf2 ** 2 where SAIL has 1 - rinf^2 e2, and the library reproduces the
 * reference's line.  The isolated canopy therefore does not conserve energy: at LAI -> 0 tau_dd -> 1 / (1 + rinf^2), not 1, and
 * fAPAR does not go to 0 with LAI (3e-4 at LAI = 1e-6); outside the PAR range a_s and a_d go slightly negative.  The products
 * are defined on the model the reflectances come from (albedo_* are weighted means of the very rsd / rdd it materialises), and
 * no physical limit is promised.
 * Order of summation.  The two denominators are summed once in spart_ctx_create, float64, i ascending.  A numerator is four
 * interleaved partial sums p_r over i = r (mod 4), each with i ascending from 0.0 and one fused multiply-add per band,
 * p = fma(Ea_i, x_i, p), joined as (p_0 + p_1) + (p_2 + p_3); then one IEEE division.  The fCover sum runs j ascending with a
 * multiplication and an addition per class.  A row's five values are therefore the same bits wherever the row stands in
 * whatever batch.
 * params: spart_run_batch's columns; params[0 ... 21] must not be NULL, params[22 ... 26] are not read and may be.  out: each
 * member (B,) device memory, optional.  The workspace is spart_workspace_bytes(ctx, SPART_F64, B).  Refused before anything is
 * launched or written, SPART_ERR_INVALID: a NULL out; with B > 0 all five outputs NULL, a NULL params or a NULL among
 * params[0 ... 21] (the message names the first).  B = 0 launches nothing.  Float64 only; the prelude is the literal one.
 * How (csrc/spart_products.h): the prelude's leaf, soil and canopy constants, then one kernel, lane = sample, the band
 * wave-uniform; its canopy solve (canopy_flux) computes the four flux terms and nothing that depends on the view direction.
 * Added WITHOUT a new interface number, by spart_refine_srf's rule: one more symbol and one new struct. */
typedef struct spart_products_out {
  double *fapar_bs, *fapar_ws, *albedo_bs, *albedo_ws, *fcover; /* each (B,) device, optional */
} spart_products_out;
int spart_products(spart_ctx *ctx, int64_t B, const double *const params[SPART_NPARAM], const spart_products_out *out,
                   void *workspace, size_t workspace_bytes, void *stream);

/* The forward model made DIFFERENTIABLE: the vector-Jacobian product of the sensor columns with respect to up to 16 free
 * parameters, by bounded central differences, without ever storing a Jacobian -- what torch.autograd needs to put the model
 * behind a network or under torch.optim (spart_amd.SpartLayer).  base, free_cols, lo, hi are spart_refine's.  gy[c] is the
 * gradient of the caller's loss with respect to column c (0 R_TOC, 1 R_TOA, 2 L_TOA), (M, nb) float64 on the device, or NULL
 * for a column the loss does not read.  grad (M, F): dLoss / d free parameter.
 * Definition (tools/vjp_defined.py is the same text in numpy), per observation m, float64, every written operation one rounded
 * operation, no FMA contraction, IEEE division:
 *   point     x_f = clip(base[free_f][m], lo_f, hi_f) (spart_refine's clip: a NaN stays a NaN);  h_f = rel_step * (hi_f - lo_f)
 *   steps     a_f = x_f + h_f; if a_f > hi_f: a_f = hi_f.   b_f = x_f - h_f; if b_f < lo_f: b_f = lo_f.  The difference is
 *             central inside the box and one-sided on a bound; rel_step <= 0.5 gives a_f - b_f >= h_f > 0 always (but for the
 *             rounding of x_f + h_f and x_f - h_f: a step below the spacing of the doubles at x_f is the caller's to avoid)
 *   rows      2 F rows and no centre row: p_f^+ is base_m with every free column at x and column free_f at a_f, p_f^- the same
 *             with b_f.  Y^+_(c,f), Y^-_(c,f) (nb,) are column c of those rows, bit for bit what
 *             spart_run_batch(SPART_F64, prune_unused_bands = 1) returns for them (thermal inputs at their defaults, no rdry_in /
 *             lidf_in, fast_prelude and nlayers honoured); with band_model 1 the *_srf column instead
 *   sum       s_f = 0.0; for c = 0, 1, 2 with gy[c] != NULL, in that order, for j ascending: g = gy[c][m, j]; g == 0 skips the
 *             band (Y may be NaN there); otherwise d = Y^+_(c,f)[j] - Y^-_(c,f)[j] and s_f = s_f + g * d, one multiplication
 *             and one addition.  grad[m, f] = s_f / (a_f - b_f)
 *   status    there is none: a NaN parameter or a non-finite g propagates by IEEE into that row's grad and nowhere else
 * Consequences (a row's column is a pure function of its own 27 parameters).  A row's gradient is the same bits wherever the row
 * stands in whatever batch or chunk.  A block of zeros for a column is NULL for it, bit for bit.  The gradient is that of the
 * CLIPPED point: a parameter outside its bounds gets the one-sided slope at the bound (straight through the clip).
 * Observations go in chunks of 2^19 / (2 F), ONE forward call of 2 F Mc rows per chunk.  spart_vjp_workspace_bytes is 0 exactly
 * for refused sizes (NULL or sensorless context, M outside 1 ... 2e9, F outside 1 ... 16); with Mc = min(M, 2^19 / (2 F)) and
 * R = 2 F Mc it is (each term rounded up to 256 bytes)
 *   8 * 27 R  +  3 * 8 R nb  +  forward scratch of R rows  +  8 Mc F:
 * one chunk's forward block and its denominators a_f - b_f, constant in M once M >= 2^19 / (2 F).
 * Everything is queued on `stream`; nothing synchronises.  Refused before anything is launched or written: SPART_ERR_INVALID
 * for a NULL context; F outside 1 ... 16; NULL free_cols / lo / hi; nlayers; a free column out of range or named twice, bounds
 * not finite lo < hi (spart_refine's checks in its order); then a NULL opt; then band_model outside 0 / 1; then rel_step
 * negative, not finite or above 0.5; then a NULL gy, or all three entries NULL; then, with band_model 1, more than one entry
 * (the SRF forward call writes one column); then a NULL grad; then M < 0 or M > 2e9; then, with M > 0, a NULL base or base column
 * (the first named).  Then SPART_ERR_NOSENSOR, then (M = 0 launches nothing) SPART_ERR_WORKSPACE.
 * How (csrc/spart_vjp.h): k_vjp_init writes the table and the denominators, the forward call is the unchanged float64 pruned
 * path, k_vjp_reduce stages tiles of 16 bands of g (Y^+ - Y^-) through LDS and one lane per (observation, f) adds them in
 * order into a register: no atomics.  Forward-mode products, second derivatives, gradients with respect to columns that are not
 * free, to the thermal inputs, rdry_in or lidf_in, and F > 16 are out of scope.  Added WITHOUT a new interface number, by
 * spart_refine_srf's rule: two symbols, one struct. */
typedef struct spart_vjp_opt {
  int32_t band_model;    /* 0 centre columns, 1 SRF-convolved columns */
  int32_t fast_prelude;  /* as spart_materialize.fast_prelude */
  int32_t nlayers;       /* as spart_materialize.nlayers, 0 = 60 */
  double  rel_step;      /* 0 = 1e-3; otherwise finite, in (0, 0.5] */
} spart_vjp_opt;
size_t spart_vjp_workspace_bytes(const spart_ctx *ctx, int64_t M, int F);
int spart_vjp(spart_ctx *ctx, int64_t M, const double *const base[SPART_NPARAM], int F,
              const int32_t *free_cols /* HOST */, const double *lo, const double *hi /* HOST (F,) */,
              const double *const gy[3] /* device, each NULL or (M, nb): dLoss/dR_TOC, dR_TOA, dL_TOA */,
              const spart_vjp_opt *opt, double *grad /* device (M, F) */,
              void *workspace, size_t workspace_bytes, void *stream);

/* PROSPECT INVERSION: bounded Levenberg-Marquardt fits of up to nine leaf parameters against measured leaf reflectance and / or
 * transmittance on the 2001-band grid (integrating-sphere spectra of LOPEX / ANGERS-type collections), one fit per leaf.  No
 * sensor is involved (a context without one serves; there is no SPART_ERR_NOSENSOR case) and no workspace.
 * leaf[9] is spart_prospect_batch's order (Cab, Cdm, Cw, Cs, Cca, Cant, N, PROT, CBC), each (M,) float64 on the device: the start
 * rows.  free_cols: F distinct entries of 0 ... 8, 1 <= F <= 9, with bounds lo / hi (host).  obs_refl, obs_tran: dense (M, 2001)
 * float64 on the device; either may be NULL, not both.  w_refl / w_tran: NULL (weight 1 on every band of that array), or (2001,)
 * with weights_per_obs 0, or (M, 2001) with 1; only for an observation array that is given.  A weight of exactly 0 skips the
 * band, and the observation may be NaN there.
 * Definition (tools/refine_leaf_defined.py is the same text in numpy): spart_refine's text word for word, per leaf m, float64,
 * every written operation one rounded operation, no FMA contraction, IEEE division and square root, with these substitutions.
 *   rows, Y   p_0 is the leaf's nine parameters with the free ones at the trial t; p_f is p_0 with free[f-1] moved by s_f h_f
 *             (h_f = rel_step (hi_f - lo_f); s_f = +1 if t_f + h_f <= hi_f else -1).  Y_0 ... Y_F are the (refl, tran) spectra
 *             of those rows: leaf_band<double> (csrc/spart_math.h) of the row's leaf constants, which are formed exactly as
 *             the prelude's PRE_LEAF part forms them (the PROSPECT-PRO rule, 1 / N, c / N, N - 1)
 *   band sums every sum over bands -- the trial cost, each A_ab, each g_a, the sums inside std's A -- is 64 lane partials plus
 *             a fixed join.  Partial p_l starts at 0.0 and takes the bands i = l, l + 64, ... < 2001 in ascending order; at
 *             each band the reflectance term first, then the transmittance term; a term is skipped if its array is absent or
 *             its weight is 0.  The terms: c = c + (w d) d with d = Y_0 - obs;  A_ab = A_ab + (w J_a) J_b (a >= b);
 *             g_a = g_a + (w J_a) r with r = Y_0 - obs and J_f = (Y_f - Y_0) / (s_f h_f).
 *             Join: for d = 32, 16, 8, 4, 2, 1: p_l = p_l + p_(l+d) for l < d; the sum is p_0.
 *             The prior's terms (c + (p e) e; A_aa + p_a; g_a + p_a e_a; e = t - mu, a weight of 0 skipped) are added after
 *             the join, in ascending order
 *   the rest  is spart_refine's: x = t = clip(start); n_iter + 1 evaluations, no early exit; the trial is accepted when
 *             c_t < c; lambda / 10 on an accept and * 10 on a reject within [1e-12, 1e12]; D_a = A_aa if A_aa > 0 else 1;
 *             (A + lambda diag D) delta = -g by Cholesky, a failed factorisation or a non-finite delta gives delta = 0;
 *             t = clip(x + delta); cost <= cost0; std from the undamped A of the last accepted point (NaN when its
 *             factorisation fails).  A dead leaf -- a negative, NaN or infinite weight on any band of a given weights array or in
 *             its prior, or a start cost not < +inf -- has n_accept = -1, std NaN, x the clipped start and cost = cost0
 *   y         y_refl, y_tran are the spectra at the returned x from one closing pass; no claim is made that they equal the
 *             in-loop Y_0 bit for bit
 * A leaf's outputs depend on nothing but its own inputs: the same bits at any position of any batch.
 * Everything is queued on `stream`; nothing synchronises; M = 0 launches nothing.  Refused before anything is launched or
 * written, each SPART_ERR_INVALID, in this order: a NULL ctx; F outside 1 ... 9; NULL free_cols, lo or hi; a free column outside
 * 0 ... 8 or named twice; bounds not finite with lo < hi; a NULL opt; n_iter outside 0 ... 100; rel_step or lambda0 negative or
 * not finite; weights_per_obs outside 0 / 1; exactly one of prior_mean / prior_weight NULL; prior_per_obs outside 0 / 1; both
 * observation arrays NULL; a weights array for a NULL observation array; a NULL out, out->x or out->cost; M < 0 or M > 2e9;
 * with M > 0 a NULL leaf or leaf column (the first is named).
 * How (csrc/spart_refine_leaf.h): k_refine_leaf<F>, one wave per leaf with its lanes along the bands, the leaf model and the
 * Levenberg-Marquardt step fused, all n_iter + 1 evaluations in one launch, no spectra in memory.  Fitting BSM or SAILH stage
 * spectra, float32, the thermal inputs, kChlrel as an observation and band-correlated noise are out of scope.  Added WITHOUT a
 * new interface number, by spart_refine_srf's rule: one symbol, two structs. */
typedef struct spart_leaf_fit_opt {
  int32_t n_iter;            /* 0 ... 100 */
  int32_t weights_per_obs;   /* 0: each weights array NULL or (2001,); 1: (M, 2001) */
  double  rel_step;          /* 0 = 1e-3 */
  double  lambda0;           /* 0 = 1e-2 */
  int32_t prior_per_obs;     /* 0: (F,), 1: (M, F) */
  const double *prior_mean, *prior_weight;   /* device; both NULL = no prior */
} spart_leaf_fit_opt;
typedef struct spart_leaf_fit_out {          /* device; x and cost required, the rest optional */
  double *x, *cost, *cost0, *std; int32_t *n_accept; double *y_refl, *y_tran;   /* (M,F) (M,) (M,) (M,F) (M,) (M,2001) (M,2001) */
} spart_leaf_fit_out;
int spart_refine_leaf(spart_ctx *ctx, int64_t M, const double *const leaf[9], int F, const int32_t *free_cols /* HOST */,
                      const double *lo, const double *hi /* HOST (F,) */, const double *obs_refl, const double *obs_tran,
                      const double *w_refl, const double *w_tran, const spart_leaf_fit_opt *opt,
                      const spart_leaf_fit_out *out, void *stream);

/* Measurement aid (bench.py): when enabled, spart_run_batch brackets each of its kernels with HIP events recorded on
 * the stream the kernel runs on, for up to max_calls calls (max_calls = 0 disables).  spart_profile_read_stages waits for
 * them and returns the summed milliseconds per stage -- [0] prelude (per-sample constants), [1] the fused full-band kernel
 * (PROSPECT + BSM + SAILH over all 2162 bands, the dominant one; includes the band-mean reduction when requested),
 * [2] the column kernel (canopy model at the sensor bands, interpolation, SMAC, TOC->TOA) -- and the number of timed
 * calls; spart_profile_read returns stage [1] only. */
#define SPART_NSTAGE 3
int spart_profile_enable(spart_ctx *ctx, int max_calls);
int spart_profile_read(spart_ctx *ctx, double *total_ms, int *ncalls);
int spart_profile_read_stages(spart_ctx *ctx, double stage_ms[SPART_NSTAGE], int *ncalls);

/* Knobs.  None of them changes a result (the one exception is marked); defaults are what every number in DESIGN.md was
 * measured with.
 *   environment, read by the library:
 *     SPART_ROCTX=1          push / pop ROCTX ranges around the stages of spart_run_batch when a roctx library can be dlopen'ed
 *     SPART_SIDE_STREAM=0    read at spart_ctx_create: run the column kernels on the caller's stream instead of a side stream
 *     SPART_CHUNK=<n>        samples per workgroup of the band kernels (tuning sweeps; default: chosen from B)
 *   environment, read by the Python loader / build script (spart_amd/_lib.py, build.py):
 *     SPART_HIP_LIB=<path>   load another build of this ABI (A/B timing, tools/ab_bench.py)
 *     SPART_FAST_MATH=0      build with IEEE division / libm transcendentals instead of v_rcp / v_exp / v_log + Newton steps
 *                            (CHANGES results at the 1e-15 (float64) / 1e-7 (float32) level; parity is tested with the default)
 *   A/B of a tuning constant (a constexpr in csrc/, next to its measurement): edit it on a branch, build each tree with
 *   build.build(out=...) and time the two libraries with tools/ab_bench.py.
 */

#ifdef __cplusplus
}
#endif
#endif /* SPART_HIP_H */
