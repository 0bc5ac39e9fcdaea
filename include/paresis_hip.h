/*
 * paresis_hip.h -- C ABI of libparesis_hip.so: the MI355X (gfx950) image-formation hot path of an X-ray
 * speckle-propagation simulator, drop-in for the numerical kernels behind
 * Experiment.computeSampleAndReferenceImages_{Fresnel,RT} of quenotl/PARESIS.
 *
 * The reference has no FFI layer: its boundary is the Python call surface of CodePython/{Experiment,Sample,
 * Detector,refractionFileNumba2,refractionFileNumba,getk}.py.  Each entry point below names the reference
 * function (file:line, relative to CodePython/) whose array work it replaces; the Python modules under paresis_amd/ keep the reference's
 * names and signatures on top of this ABI (see INTEGRATION.md for the ctypes binding a maintainer would add).
 *
 * Conventions
 *   - every pointer named T/I/wave/phi/out/... is a DEVICE pointer (HBM); "host array" is said explicitly;
 *   - images are row-major [Nx][Ny] (numpy C order: axis 0 = "x" of the reference), float32 / interleaved complex64;
 *     the optional explicit phase is float64 (fp32 cannot hold kilo-radian phases to 1e-5);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call is asynchronous on it, performs
 *     no host synchronisation and allocates nothing the caller must free (plans own their work buffers);
 *   - return value: 0 = ok, <0 = invalid argument (PSX_E_*), >0 = hipError_t or 1000+rocfft_status;
 *     psx_last_error() returns a thread-local description of the last failure;
 *   - thread model: one host thread per GPU/process; plans are not shared between threads.
 *
 * Materials: an object is a stack of thickness maps T[m] (metres, float32, [Nx][Ny]) with two per-map coefficients,
 *   cphase[m] (rad/m, added to the phase:  phi += cphase[m]*T[m];  the reference's -k*delta, Sample.py:279,348) and
 *   catt[m]   (1/m, log-attenuation:       log a += catt[m]*T[m]; -k*beta for a wave, -2*k*beta for an intensity,
 *   Sample.py:279,347).  Products and sums over m are formed in float64 on the device, then range-reduced.
 */
#ifndef PARESIS_HIP_H
#define PARESIS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSX_MAX_MAT 8
#define PSX_MAX_DIST 8
#define PSX_MAX_SRC 16    /* source waves per psx_fresnel_propagate_sources / images per psx_accumulate_many_f32 call */

#define PSX_E_ARG (-1)      /* bad argument (null pointer, size, count) */
#define PSX_E_STATE (-2)    /* plan/shape mismatch */
#define PSX_E_UNSUPPORTED (-3)

/* bits of the device status word (psx_status_*) */
#define PSX_STATUS_NONFINITE 1u   /* NaN or |v| > 1e50 in a refracted image: refractionFileNumba2.py:81-82 raises */

typedef struct psx_fresnel_plan psx_fresnel_plan;
typedef struct psx_detector_plan psx_detector_plan;
typedef struct psx_integrate_plan psx_integrate_plan;

typedef struct { float re, im; } psx_c64;

/* library / build identification; psx_abi_version() changes when a signature changes */
int psx_abi_version(void);
const char *psx_last_error(void);
/* 1 when the code object for the current device (gfx950) is loadable, else 0 with psx_last_error() set */
int psx_device_ok(void);
/* Diagnostics: the shader clock (MHz) the device runs at under load right now -- a 30 us spin on every CU, issued on `stream` behind
 * whatever is queued there, bracketed by the shader-clock and the constant 100 MHz counters; synchronises the stream.  bench.py
 * reports it next to its timings: the boxes of a pool differ by more than 10 % in what they sustain. */
int psx_clock_probe(float *mhz, void *stream);

/* ---- K1: AnalyticalSample.setWave (Sample.py:248-282) ------------------------------------------------------
 * wave_out[p] = amp * wave_in[p] * exp(sum_m catt[m]*T[m][p]) * exp(i * sum_m cphase[m]*T[m][p]),  p < n.
 * wave_in may be NULL (unit wave).  T is a HOST array of nmat device pointers.  In place (wave_out==wave_in) is ok. */
int psx_transmit_wave_c64(const psx_c64 *wave_in, float amp, const float *const *T, const double *cphase,
                          const double *catt, int nmat, psx_c64 *wave_out, int64_t n, void *stream);

/* ---- K2: AnalyticalSample.setWaveRT (Sample.py:285-351, scalar dark field) ------------------------------------
 * I_out[p] = I0 * I_in[p] * exp(sum_m catt[m]*T[m][p]);   phi_out[p] = phi_in[p] + sum_m cphase[m]*T[m][p].
 * I_in may be NULL (ones); phi_in may be NULL (zeros); phi_out may be NULL (phase not wanted); I_out may be NULL. */
int psx_transmit_rt_f32(const float *I_in, float I0, const float *const *T, const double *cphase, const double *catt,
                        int nmat, float *I_out, const double *phi_in, double *phi_out, int64_t n, void *stream);

/* ---- material fold: a stack of more than PSX_MAX_MAT maps as three (Sample.py:279, 347-348 loop over any number) ----
 * P = sum_m cphase[m]*T[m][p] in float64 (the fma order of every consumer), A = sum_m catt[m]*T[m][p];
 * P_hi[p] = (float)P, P_lo[p] = (float)(P - P_hi[p]), A_out[p] = (float)A.  The stack [P_hi, P_lo, A] with cphase (1, 1, 0)
 * and catt (0, 0, 1) gives every consumer the same exponents to ~1e-14 relative: the hi/lo pair carries a phase of
 * hundreds of radians past float32.  T: HOST array of nmat <= PSX_MAX_FOLD device pointers; one launch reads each once. */
#define PSX_MAX_FOLD 64
int psx_fold_materials_f32(const float *const *T, const double *cphase, const double *catt, int nmat, float *P_hi,
                           float *P_lo, float *A_out, int64_t n, void *stream);

/* acc[p] (+)= scale * img[p] * exp(sum_m catt[m]*T[m][p])  -- plate attenuation + energy accumulation
 * (Experiment.py:351-358, 478-483).  accumulate: 0 store, 1 add.  nmat may be 0. */
int psx_accumulate_f32(float *acc, const float *img, float scale, const float *const *T, const double *catt, int nmat,
                       int accumulate, int64_t n, void *stream);

/* The same, also reducing what it adds (Experiment.py:360-361 / 485-486: np.mean of the per-energy reference image feeds
 * the intensity-weighted mean energy): with v[p] = scale*img[p]*exp(sum catt*T[p]) and S = sum_p v[p], the kernel adds S and
 * weight*S (weight = the energy) into `sums`, a device float64 array of PSX_SUM_SLOTS slots of PSX_SUM_STRIDE doubles
 * (128 bytes apart, so that the atomics of different workgroups do not serialise on one line), caller-zeroed:
 *   sum_s sums[s*PSX_SUM_STRIDE + 0] = sum of S over the calls,   sum_s sums[s*PSX_SUM_STRIDE + 1] = sum of weight*S.
 * acc may be NULL (sums only). */
#define PSX_SUM_SLOTS 32
#define PSX_SUM_STRIDE 16
int psx_accumulate_sum_f32(float *acc, const float *img, float scale, const float *const *T, const double *catt, int nmat,
                           int accumulate, int64_t n, double *sums, double weight, void *stream);
/* The same for the images of n_img <= PSX_MAX_SRC energies in ONE pass (the energies of a detector bin): acc (+)= sum over e of
 * scale[e] * imgs[e] * exp(sum_i catt[e*nmat + i] * T[i]), added in the order of e exactly as one psx_accumulate_sum_f32 call
 * per energy would (bit-identical float32 result); sums (may be NULL) += (sum of all terms, sum of weight[e] * term).
 * acc may be NULL (sums only).  imgs, scale, catt, weight: host arrays. */
int psx_accumulate_many_f32(float *acc, const float *const *imgs, const float *scale, int n_img, const float *const *T,
                            const double *catt, int nmat, int accumulate, int64_t n, double *sums, const double *weight,
                            void *stream);

/* ---- K9-K13: fastRefraction (refractionFileNumba2.py:25-86; variant v1: refractionFileNumba.py:11-68) ----------
 * Source intensity  I_src = I0 * I_in * exp(sum catt*T)          (I_in may be NULL = ones; fused K2)
 * Phase             phi   = phi_in + sum cphase*T                 (phi_in float64, may be NULL)
 * Displacement      D     = grad(phi) * dscale, np.gradient(edge_order=2) with unit spacing, i.e. the caller passes
 *                   dscale = z / k / (h*M) / h  (RF2:54-56);  |D|<1e-12 -> 0;  |Dx|>clamp_x or |Dy|>clamp_y -> I=0,
 *                   that component = 0 (RF2:59-64: clamp = Nx,Ny for v2, 1e3 for v1).
 * Output            I_out[Nx][Ny] (+)= out_scale * bilinear scatter of I_src by D on a grid padded by `margin`
 *                   (15 for v2, 10 for v1), cropped back (RF2:65-78, loop RF2:198-263).
 * Dx_out/Dy_out     optional [Nx+2*margin][Ny+2*margin] float32 (zero margins), as the reference returns them.
 * I_mut             optional: the reference zeroes clamped entries of its INPUT intensity in place (RF2:61-62);
 *                   pass I_in here to reproduce that, NULL otherwise.
 * status            optional device word; PSX_STATUS_NONFINITE is OR-ed in when the output holds NaN/inf.
 * workspace         device scratch of psx_refract_workspace_bytes(Nx,Ny) bytes (far-ray lists; with psx_set_deterministic on,
 *                   also the scratch words of the order-independent replay), caller-owned, no initial state needed.
 */
size_t psx_refract_workspace_bytes(int Nx, int Ny);
/* Gather halo of the tile kernel: 4, 6, 8, 12 or 16 pixels (default 4; the two widest for grids whose rays travel far in study pixels); a setting of the CALLING HOST THREAD (one thread per GPU).  A tile gathers every ray of its window (tile + halo)
 * that lands in it, however long; what remains for the slower far-ray replay are the shares whose source lies outside
 * the window of the target's tile.  A pure speed knob: results are identical up to the float-atomics order of those. */
int psx_refract_set_halo(int halo);
int psx_refract_f32(const float *I_in, float I0, const float *const *T, const double *cphase, const double *catt,
                    int nmat, const double *phi_in, float *I_out, float out_scale, int accumulate, float *Dx_out,
                    float *Dy_out, float *I_mut, int Nx, int Ny, int margin, double dscale, double clamp_x,
                    double clamp_y, unsigned *status, void *workspace, void *stream);
/* fastRefractionDF's split by its width map (refractionFileNumba2.py:147-150: I_nodf = I where DF == 0, I_df = I where
 * DF != 0) and the refraction of both halves (RF2:153-154) in one call: I_out_zero receives the refraction of the sources
 * where mask == 0, I_out_nonzero of those where mask != 0.  A tile is staged ONCE for both; a half runs its deposit loop only
 * where the tile's window holds a source of its side.  With the thickness maps as the source of intensity and phase, the
 * dark-field branch of the chain (EXP:469-473) needs neither the transmitted (I, phi) pair nor the two halves of the split in
 * memory.  mask: [Nx][Ny] float32 (the width map in pixels).  The phase comes from the thickness maps (nmat > 0; phi_in must
 * be NULL: the argument keeps the call's shape that of psx_refract_f32).  No displacement maps, no input mutation; workspace:
 * psx_refract_multi_workspace_bytes(Nx, Ny, 2); everything else as psx_refract_f32. */
int psx_refract_split_f32(const float *I_in, const float *mask, float I0, const float *const *T, const double *cphase,
                          const double *catt, int nmat, const double *phi_in, float *I_out_zero, float *I_out_nonzero,
                          float out_scale, int accumulate, int Nx, int Ny, int margin, double dscale, double clamp_x,
                          double clamp_y, unsigned *status, void *workspace, void *stream);

/* Propagation-distance batch (BASELINE.json north_star: "propagation-distance batches"; the reference would call
 * Experiment.refraction, Experiment.py:255-277, once per distance on the same (I, phi)): ndist <= PSX_MAX_DIST
 * refractions of ONE source (same I_in/I0/T/phi_in) with displacement scales dscale[d] into the distinct images
 * I_out[d] (host arrays of ndist entries), in one launch per kernel -- the thickness maps are read and the
 * transmission evaluated once per tile instead of once per distance.  Each image is bit-identical to the one
 * psx_refract_f32 gives for that distance (up to the float-atomics order of far rays).  Dx_out/Dy_out/I_mut are
 * only accepted with ndist == 1.  workspace: psx_refract_multi_workspace_bytes(Nx, Ny, ndist) bytes. */
size_t psx_refract_multi_workspace_bytes(int Nx, int Ny, int ndist);
int psx_refract_multi_f32(const float *I_in, float I0, const float *const *T, const double *cphase, const double *catt,
                          int nmat, const double *phi_in, float *const *I_out, float out_scale, int accumulate,
                          float *Dx_out, float *Dy_out, float *I_mut, int Nx, int Ny, int margin, const double *dscale,
                          int ndist, double clamp_x, double clamp_y, unsigned *status, void *workspace, void *stream);
/* A batch of n <= PSX_MAX_SRC refractions over the SAME thickness maps in one launch per kernel -- the energies of a detector
 * bin (Experiment.py:448-486 loops over them): refraction e has its own input image I_in[e] (all or none; none = the uniform
 * I0[e]), coefficients cphase/catt[e*nmat + i], displacement scale dscale[e] and output image I_out[e]; one distance each, no
 * displacement maps.  Every image is what psx_refract_f32 gives for that refraction (far rays apart: float atomics).
 * workspace: psx_refract_batch_workspace_bytes(Nx, Ny, n) bytes. */
size_t psx_refract_batch_workspace_bytes(int Nx, int Ny, int n);
int psx_refract_batch_f32(int n, const float *const *I_in, const float *I0, const float *const *T, const double *cphase,
                          const double *catt, int nmat, float *const *I_out, float out_scale, int accumulate, int Nx, int Ny,
                          int margin, const double *dscale, double clamp_x, double clamp_y, unsigned *status, void *workspace,
                          void *stream);

/* Order-independent scatter (the reference's scatter is a single-threaded raster loop, RF2:217-263; the
 * tile gathers are fixed point and reproducible as they are, but far rays and psx_fastloop_f32 deposit with global float
 * atomics in arrival order, and a last-bit difference can flip a Poisson draw downstream).  With on != 0 the far-ray replay of
 * psx_refract_f32 / _multi_f32 / _batch_f32 sums in fixed point: the tile kernel clears the 64-bit scratch words a far ray may
 * reach when it lists the ray; the replay adds every share as an integer -- ONE unit per call, 2^-30 of the power of two
 * above the largest intensity the call stages, so every share fits whatever tile it lands in -- with a returning atomic (the
 * thread that reads back zero was first at that pixel and notes the pixel in its list's fold table); a second pass adds each
 * pixel's complete sum ONCE to the float image.  Two runs of the same call are then bitwise equal, whatever the GPU count.
 * One atomic per share, as in the float form.  Allocates nothing and synchronises nothing: the scratch ([ndist][Nx*Ny] words)
 * is part of the caller's workspace, needs no initial state, and psx_refract_*_workspace_bytes() includes it WHILE THE MODE
 * IS ON (set the mode, then size the workspace).  psx_fastloop_f32, which has no workspace argument, keeps the allocating
 * form (hipMalloc + a stream synchronisation per call).  A setting of the calling host thread, off by default in the library;
 * the Experiment class turns it on around its ray-tracing chain unless exp_dict['reproducible'] is False (measured cost:
 * DESIGN.md section 4.3).  psx_get_deterministic returns the calling thread's setting (callers that restore it). */
int psx_set_deterministic(int on);
int psx_get_deterministic(void);
/* Optional: the fixed-point unit of the order-independent replay from the CALLER's intensity scale instead of the call's measured
 * maximum -- scale > 0: one unit = 2^-30 of the power of two above 64 * scale (a share up to 2^10 times that is taken -- 2^11 of them
 * fit a pixel's sum --; beyond, PSX_STATUS_NONFINITE is raised); the tile kernels then send no maximum and the call needs no memset node (4.7 us per call at
 * 4096^2).  The sums are quantised to the unit whatever the image holds, so the scale should be the image's order of magnitude
 * (the Experiment class passes the incident intensity per study pixel).  0 (default): measure.  A setting of the calling thread. */
int psx_set_deterministic_scale(float scale);
/* the calling thread's setting (callers that restore it: a nested scope must not lose the outer scope's scale) */
float psx_get_deterministic_scale(void);

/* The raw scatter loop on explicit displacement fields: fastloopNumba (refractionFileNumba2.py:198-263).
 * I, Dx, Dy, I2 are [Nx][Ny]; I2 is accumulated into (float atomics; order-dependent in the last bits). */
int psx_fastloop_f32(const float *I, const float *Dx, const float *Dy, float *I2, int Nx, int Ny, void *stream);

/* ---- K3-K8: Experiment.wavePropagation (Experiment.py:219-252) ------------------------------------------------
 * A plan fixes the study grid [Nx][Ny] and the reflect margin (15, EXP:236) and owns the padded work buffers.
 * engine: 0 = auto, 1 = rocFFT on the padded grid (pad -> FFT2 -> chirp -> IFFT2 -> crop, any size),
 *         2 = LDS-resident FFT convolution (row pass + column pass, the padded spectrum never touches HBM; lines longer
 *             than one LDS transform, N > 4593, as a partitioned convolution).  Auto picks 2 for every supported grid. */
#define PSX_ENGINE_AUTO 0
#define PSX_ENGINE_ROCFFT 1
#define PSX_ENGINE_LDS 2
int psx_fresnel_plan_create(int Nx, int Ny, int margin, int max_dist, int engine, psx_fresnel_plan **plan);
int psx_fresnel_plan_destroy(psx_fresnel_plan *plan);
/* engine actually selected (PSX_ENGINE_ROCFFT / PSX_ENGINE_LDS) */
int psx_fresnel_plan_engine(const psx_fresnel_plan *plan);
/* bytes of device memory the plan owns */
size_t psx_fresnel_plan_bytes(const psx_fresnel_plan *plan);
/* on != 0: the LDS engine's one-transform passes (N <= 4593) hand their line groups to the workgroups through queues (the
 * share of a workgroup is an atomic counter it claims from; a workgroup whose share is done steals from the others of its
 * XCD) instead of equal static shares.  Static shares are ~4 % faster on a GPU the call has to itself, and
 * TWICE as slow as soon as one CU is busy with anything else when a pass starts (its 256 workgroups need a whole CU each:
 * the one that cannot start waits for another to finish its whole share) -- e.g. the copy kernels of an RCCL transfer that
 * overlaps the computation.  Same results bit for bit.  Default off; no effect on the other engine paths. */
int psx_fresnel_plan_work_queue(psx_fresnel_plan *plan, int on);

/* Propagate ONE input wave to n_dist distances, e.g. EXP:341 and EXP:349 (shared across the distances: the transmitted
 * source wave in the LDS engine, the forward 2-D transform as well in the rocFFT engine).
 *   input  psi = amp * wave_in * transmission(T, cphase, catt)          (wave_in may be NULL = unit wave; fused K1)
 *   for d < n_dist:  out_d = exp(i*gphase[d]) * IDFT2( exp(-i*a[d]*(u^2+v^2)) * DFT2(reflect_pad(psi)) ) cropped,
 *                    u_i = (i - Px/2)*du_x, v_j = (j - Py/2)*du_y  with du = 2*pi/(N*h) from the UN-padded N (EXP:246-247),
 *                    a[d] = z/(2*k*M), gphase[d] = k*z/M  (EXP:250);  a[d] == 0 means "z == 0": out_d = psi (EXP:233).
 *   wave_out[d]  (host array of device pointers, entries may be NULL): complex result [Nx][Ny]
 *   inten_out[d] (host array of device pointers, entries may be NULL): inten_out[d] (+)= inten_scale[d]*|out_d|^2 (K8)
 */
int psx_fresnel_propagate(psx_fresnel_plan *plan, const psx_c64 *wave_in, float amp, const float *const *T,
                          const double *cphase, const double *catt, int nmat, int n_dist, const double *a,
                          const double *gphase, double du_x, double du_y, psx_c64 *const *wave_out,
                          float *const *inten_out, const float *inten_scale, int accumulate, void *stream);
/* The same for n_src <= PSX_MAX_SRC source waves over the SAME thickness maps in one call -- the energies of a detector bin
 * (EXP:317-361 loops over them): source s has its own input wave wave_in[s] (the array or an entry may be NULL = unit wave),
 * amplitude amp[s] and coefficients cphase/catt[s*nmat + i]; pair (s, d) has its own a, gphase, outputs and scale at index
 * s*n_dist + d.  Every pair's result is exactly what psx_fresnel_propagate gives for that source (nothing is accumulated:
 * each pair owns its output).  On grids too small to fill the chip (fewer line groups than CUs) the LDS engine runs the
 * whole batch in three launches -- the pairs are one more axis of its work items -- when n_src*n_dist <= 32; otherwise the
 * sources are taken one after the other.  The first batched call of a plan allocates its batch buffers (not under capture). */
int psx_fresnel_propagate_sources(psx_fresnel_plan *plan, int n_src, int n_dist, const psx_c64 *const *wave_in, const float *amp,
                                  const float *const *T, const double *cphase, const double *catt, int nmat, const double *a,
                                  const double *gphase, double du_x, double du_y, psx_c64 *const *wave_out,
                                  float *const *inten_out, const float *inten_scale, void *stream);

/* ---- K14-K19: Detector.detection (Detector.py:79-119), resize (:185-198), create_gaussian_shape (:201-220) -----
 * reflect-pad 15*ov -> source blur (sigma_src study px, 0 = none) -> ov x ov block SUM -> PSF blur (sigma_psf detector
 * px, 0 = none) -> crop 15.  All stages are linear and separable; the plan holds the composed banded operators.
 * out [nx][ny] (+)= ... ; Poisson noise is a separate call (psx_poisson_f32). */
int psx_detector_plan_create(int Nx, int Ny, int ov, int nx, int ny, int margin, double sigma_src, double sigma_psf,
                             psx_detector_plan **plan);
int psx_detector_plan_destroy(psx_detector_plan *plan);
int psx_detect_f32(psx_detector_plan *plan, const float *img, float *out, void *stream);
/* The detector operator on nimg <= PSX_MAX_DETECT images of the plan's shape in one call (imgs, outs: host arrays of device
 * pointers; distinct outputs) -- the two to four images of an energy bin (Experiment.py:388-394 / 507-514).  When both stages run
 * fused the images share each launch; out[i] is bit for bit what psx_detect_f32(plan, imgs[i], outs[i]) would write. */
#define PSX_MAX_DETECT 4
int psx_detect_multi_f32(psx_detector_plan *plan, const float *const *imgs, float *const *outs, int nimg, void *stream);
/* Host-only view of one axis of the composed operator (no GPU needed): row r of the [n x N] banded matrix is
 * weights[r*wcap .. r*wcap+W) applied to study pixels start[r] .. start[r]+W.  *W_out receives the band width;
 * fails with PSX_E_ARG when it exceeds wcap. */
int psx_detector_operator_host(int N, int ov, int n, int margin, double sigma_src, double sigma_psf, int *start,
                               float *weights, int wcap, int *W_out);
/* What a plan decided, for tests and tools (host only, no GPU call, nothing about a detection changes): fills info[0 .. min(cap,
 * PSX_DETECTOR_PLAN_INFO)) and returns how many it wrote (0 for a null plan or info, or cap <= 0), in this order:
 *   0-3  band widths of the front operators of axis 0 and 1 and of the back (PSF + crop) operators of axis 0 and 1 (0 without
 *        a PSF);
 *   4-6  the fused front pair: fits (0/1), its tiles' halos are cheap (0/1), output rows per tile;
 *   7-8  the fused back pair: fits (0/1), output rows per tile;
 *   9    both back operators are plain convolutions (0/1: the PSF stage can run as a stencil);
 *   10   row pitch of the fused front's intermediate image, floats;   11  its row length, floats.
 * Whether a fused form RUNS also depends on the call: Ny % 4, the images' alignment and the "detect_4pass" switch. */
#define PSX_DETECTOR_PLAN_INFO 12
int psx_detector_plan_info(const psx_detector_plan *plan, int *info, int cap);
/* out[x][y] = sum of the s x s block of img, s = Nx/sx (Detector.resize, Detector.py:185-198) */
int psx_resize_f32(const float *img, int Nx, int Ny, float *out, int sx, int sy, void *stream);
/* out[p] = Poisson(lam[p]) drawn from a counter-based generator keyed by (seed, p)  (Detector.py:113-115;
 * the reference seeds from the wall clock, so only the distribution is reproducible).
 * Supported means: 0 <= lam <= 2^23, so that every count the sampler can reach stays below 2^24 and is an exact float32
 * integer (tests/test_gpu_poisson.py holds the distribution to the exact one from 1e-6 to 1e6).  lam <= 0 (-0.0 and -inf
 * included) and NaN give 0; a denormal lam gives 0 (its exp(-lam) is 1.0f).  Beyond the range nothing is reported -- no error,
 * no status bit -- and the value is not a Poisson draw: for a finite lam > 2^24 a float32 near lam + sqrt(lam) N(0,1), rounded
 * to the float32 grid there (spacing >= 2); for +inf a non-finite float32 (inf - inf in the candidate).  Both paths of the
 * kernel (16-byte and scalar) give the same bits there too. */
int psx_poisson_f32(const float *lam, float *out, int64_t n, uint64_t seed, void *stream);
/* The same IN PLACE on nimg <= PSX_MAX_POISSON images of n pixels in ONE launch, image i under key seeds[i] (imgs, seeds:
 * host arrays) -- the three or four detector images of an energy bin (Experiment.py:388-394).  Image i comes out exactly as
 * psx_poisson_f32(imgs[i], imgs[i], n, seeds[i]) would leave it. */
#define PSX_MAX_POISSON 8
int psx_poisson_multi_f32(float *const *imgs, const uint64_t *seeds, int nimg, int64_t n, void *stream);
/* Photon-count images as 16-bit integers for the gather of the per-position stacks (main.py:63-110 keeps every position's
 * images on one host; here they cross xGMI once): dst[p] = src[p] for counts below 65535; a larger count leaves the escape
 * code 65535 in dst and the pair (index0 + p, count) in exc[cap][2], *exc_count counting them (both device memory, the count
 * zeroed by the caller; index0 + n < 2^32).  *overflow (a device int the caller zeroed) is raised when some src[p] is not an
 * integer in [0, 2^24] or the table is full -- the caller then moves the float32 image instead, so the round trip is lossless
 * or not taken.  psx_unpack_counts_u16 is the inverse over a whole buffer: widen n pixels, then write back the exceptions
 * whose index is below n (cap = 0: none). */
int psx_pack_counts_u16(const float *src, uint16_t *dst, int64_t n, int64_t index0, int32_t *exc, int32_t *exc_count, int cap,
                        int *overflow, void *stream);
int psx_unpack_counts_u16(const uint16_t *src, float *dst, int64_t n, const int32_t *exc, const int32_t *exc_count, int cap,
                          void *stream);

/* ---- dark-field refraction, second half: the per-pixel variable-width Gaussian re-splat of
 * fastRefractionDF (refractionFileNumba2.py:168-186).  I2DF: refracted dark-field intensity, DF: dark-field width in
 * pixels at each TARGET pixel (0 = no spreading), I2: refracted non-dark-field intensity added at the end (may be NULL),
 * all [Nx][Ny] on the cropped grid; R >= round(1.5*max DF) is the largest patch half-size.  workspace:
 * psx_darkfield_workspace_bytes(Nx,Ny) bytes. */
size_t psx_darkfield_workspace_bytes(int Nx, int Ny);
int psx_darkfield_blur_f32(const float *I2DF, const float *DF, const float *I2, float *out, int Nx, int Ny, int R,
                           void *workspace, void *stream);
/* The front of fastRefractionDF in one pass (refractionFileNumba2.py:114-150): DF_px = DF_rad * num / den in float64 and in
 * that order -- RF2:114 with num = propagationDistance, den = studyPixelSize*1e-6*magnification, so that the step functions
 * of it (margin, DF > Nx/4 rule, patch sides) fall where the reference's fall --, its largest
 * value before and after the rule DF_px > limit -> 0 (RF2:135; words[0], words[1]: the doubles' bit patterns, device memory,
 * read back by the caller only when it does not know the maximum), the split of I by DF_px != 0 into I_nodf / I_df
 * (RF2:147-150) and the per-source patch table `prep` (psx_darkfield_workspace_bytes) of the re-splat, which depends on
 * the width map alone.  psx_darkfield_blur_prepared_f32 is psx_darkfield_blur_f32 on that table;
 * psx_darkfield_merge_f32: I = a + b (the caller's array after the clamped rays were zeroed in both halves, RF2:128-129);
 * psx_repad_f32: the centre [Nx][Ny] of a map padded by margin_src, re-padded with zeros to margin_dst (the displacement
 * maps fastRefractionDF returns are padded by ceil(6 max DF), RF2:117,139-140). */
int psx_darkfield_split_f32(const float *I, const double *DF_rad, double num, double den, double limit, float *I_nodf,
                            float *I_df, float *DF_px, void *prep, unsigned long long *words, int Nx, int Ny, void *stream);
int psx_darkfield_blur_prepared_f32(const float *I2DF, const float *DF, const void *prep, const float *I2, float *out, int Nx,
                                    int Ny, int R, unsigned *status, int accumulate, void *stream);   /* status: optional word, PSX_STATUS_NONFINITE (RF2:190-193); accumulate: out += result (the chain's sum over energies, EXP:478-483) */
int psx_darkfield_merge_f32(float *I, const float *a, const float *b, int64_t n, void *stream);
int psx_repad_f32(const float *src, int margin_src, float *dst, int margin_dst, int Nx, int Ny, void *stream);

/* ---- membrane thickness synthesis (next row of the scope table) -----------------------------
 * getMembraneSegmentedFromFile's sphere splat (Samples/getMembraneFromFile.py:143-159) for ONE layer:
 * out[i][j] (+)= scale * sum over spheres of 2*sqrt(r^2 - dist^2) on the cropped grid, with the reference's window and
 * placement rules.  xf, yf, rad are HOST arrays (pixels of the margin-extended grid: they come from a host-side list);
 * out is a DEVICE image.  Unlike the rest of the ABI this call synchronises the stream once (host staging buffers).
 * The rule, as tests/_membrane_oracle.py states it and tests/test_gpu_membrane.py holds all three entry points to, per pixel:
 * xi = rint(xf) (half to even), radInt = floor(r) + 1; a sphere is drawn iff r > 0, xf, yf, r are finite and
 * margin2 < xi < dimX + margin + margin2 (the same for yi); it adds 2 sqrt(r^2 - d^2) where d^2 < r^2 on the pixels of
 * [xi - radInt, xi + radInt) x [yi - radInt, yi + radInt); the map is cropped to [margin, margin + dim).  Chords are summed in
 * float64 here, so any finite radius is taken. */
int psx_membrane_f32(const double *xf, const double *yf, const double *rad, int64_t n, int dimX, int dimY, int margin,
                     int margin2, double scale, int accumulate, float *out, void *stream);

/* The same with the sphere list resident on the GPU.  The reference re-places ONE scaled, stitched list for every
 * membrane position and layer with a new integer offset (getMembraneFromFile.py:139-142); a plan takes the list once
 * (HOST arrays x, y, r in pixels of the list frame, i.e. par/pixSize before the offset), bins it by 32-pixel cell, and
 * psx_membrane_layer_f32 renders one layer at offset (offx, offy) -- xfloat = x - offx, yfloat = y - offy -- without
 * touching the host: asynchronous on the stream like the rest of the ABI.
 * The plan path sums chords in 2^-36 pixel fixed point, which sets two limits on a radius.  psx_membrane_plan_create fails with
 * PSX_E_ARG when a kept radius is 2^14 = 16384 pixels or more (a chord must stay below 2^15 pixels; psx_membrane_f32 takes such
 * a list).  A sphere of radius 2^-38 pixel or less is left out of the plan: each of its chords is at most half an accumulator
 * unit and rounds to zero, so no sum changes.  Entries with r <= 0 or a non-finite x, y or r are left out as well. */
typedef struct psx_membrane_plan psx_membrane_plan;
int psx_membrane_plan_create(const double *x, const double *y, const double *r, int64_t n, psx_membrane_plan **plan);
int psx_membrane_plan_destroy(psx_membrane_plan *plan);
/* What a plan holds and how this build stages it, for tests and tools (host only, no GPU call): fills info[0 .. min(cap,
 * PSX_MEMBRANE_PLAN_INFO)) and returns how many it wrote (0 for a null plan or info, or cap <= 0), in this order:
 *   0    spheres kept;   1-2  cells of the list frame along axis 0 and 1;   3  floor(largest kept radius) + 1;
 *   4    cell side, pixels;   5-6  tile rows and columns of the layers kernel;   7  spheres per job and batch;
 *   8    (layer, cell row) jobs staged per round;   9  layers per launch. */
#define PSX_MEMBRANE_PLAN_INFO 10
int psx_membrane_plan_info(const psx_membrane_plan *plan, int *info, int cap);
int psx_membrane_layer_f32(psx_membrane_plan *plan, int offx, int offy, int dimX, int dimY, int margin, int margin2,
                           double scale, int accumulate, float *out, void *stream);
/* Every layer of a membrane position in ONE launch (getMembraneFromFile.py:139-159 loops over nbOfLayers offsets and adds
 * into one float64 map): the chords of all nlayers offsets (offx, offy: HOST arrays) are summed as integers of 2^-36 pixel --
 * the same bits whatever the order of the list or of the layers -- and stored once, eight layers per launch (a later launch
 * adds its float32 sum to the map); nlayers = 0 stores zeros.  support (may be NULL) is the position's second map, the uniform
 * support thickness (getMembraneFromFile.py:163), filled with support_value by the first launch. */
int psx_membrane_layers_f32(psx_membrane_plan *plan, int nlayers, const int *offx, const int *offy, int dimX, int dimY,
                            int margin, int margin2, double scale, int accumulate, float *out, float *support,
                            float support_value, void *stream);

/* ---- contrast phantom (Samples/generateContrastPhantom.py): 12 tubes in a solid-water support -----------------------
 * The host derives every scalar by the generator's own expressions (paresis_amd/Samples/generateContrastPhantom.py); the
 * kernels do the per-pixel work.  Slice m (dimY x dimY, never stored) is the indicator of tube m < 12, or of the support
 * (m = 12): window rows [row0, row1) x cols [col0, col1) with (i - ci)^2 + (j - cj)^2 < rad2 in float64, the support
 * minus every tube pixel.  lines[m][c] = sum over rows r (in order) of the bilinear sample of slice m at column
 * cos*c + sin*r + off_x, row -sin*c + cos*r + off_y, zero outside the slice (skimage radon(slice, [angle]), circle=True).
 * geom [13][dimX][dimY] float32: (float)(lines[m][c] * pix_mm * 1e-3) on rows [tube_row0, tube_row1) for a tube,
 * [support_row0, support_row1) for the support, 0 elsewhere.  lines: DEVICE [13][dimY] float64, written. */
#define PSX_PHANTOM_TUBES 12
typedef struct {
    int dimX, dimY;
    double ci[PSX_PHANTOM_TUBES + 1], cj[PSX_PHANTOM_TUBES + 1];   /* centres (pixels); index 12: the support */
    int row0[PSX_PHANTOM_TUBES + 1], row1[PSX_PHANTOM_TUBES + 1];  /* half-open windows of each slice */
    int col0[PSX_PHANTOM_TUBES + 1], col1[PSX_PHANTOM_TUBES + 1];
    double rad2[PSX_PHANTOM_TUBES + 1];                            /* squared radius (pixels^2) */
    double cos_a, sin_a, off_x, off_y;                             /* radon's inverse map */
    double pix_mm;
    int tube_row0, tube_row1, support_row0, support_row1;          /* output rows (Python slice semantics, resolved) */
} psx_phantom_desc;
int psx_contrast_phantom_f32(const psx_phantom_desc *desc, double *lines, float *geom, void *stream);
/* Debug/test: the 13 slices as bytes (0/1), [13][dimY][dimY] device buffer.  Small grids only. */
int psx_contrast_phantom_slices_u8(const psx_phantom_desc *desc, uint8_t *slices, void *stream);

/* ---- labelled voxel volume: the phantom's projection model fed from memory ----------------------------------------------
 * labels [n][m][m] uint8, DEVICE: labels[z] is the slice of height z in the orientation of the phantom's slices and of
 * psx_fbp_f32's volume.  Label 0 is empty, label k + 1 is material k < nmat (a label above nmat counts as empty).
 * geom [nmat][dimX][dimY] float32 (metres) and, unless NULL, lines [nmat][dimX][dimY] float64 (voxels), DEVICE, written.
 * The host passes cos and sin of np.deg2rad(angle), c = m / 2 (integer), off_x = -c (cos + sin - 1),
 * off_y = -c (cos - sin - 1), s = study pixel / voxel and the voxel in metres.
 *   Row of study pixel (x, y):  z = n / 2 + (int)floor((double)(x - dimX / 2) * s + 0.5); outside [0, n) every material is 0.
 *   Line integral, in float64 with every product and sum rounded on its own:  cpos = (double)(y - dimY / 2) * s + (double)c,
 *   and for r = 0 .. m - 1 in ascending order  X = cos*cpos + sin*r + off_x,  Y = (-sin*cpos) + cos*r + off_y,
 *   minr, minc their floors and maxr, maxc their ceils, dr = Y - minr, dc = X - minc, tl, tr, bl, br the indicator of
 *   material k at (minr, minc), (minr, maxc), (maxr, minc), (maxr, maxc), 0 outside the slice:
 *     acc_k += (1 - dr) * ((1 - dc) * tl + dc * tr) + dr * ((1 - dc) * bl + dc * br)
 *   -- the phantom's expressions term for term (scikit-image radon of the slice, circle=True).
 *   lines[k][x][y] = acc_k,  geom[k][x][y] = (float)(acc_k * voxel_m).
 * At s = 1, m = dimY, n = dimX, cpos is exactly y and z exactly x.  The kernel applies no mask: radon's circle is the
 * loader's job, which refuses a label where (i - c)^2 + (j - c)^2 > c^2; the rotation axis is then study column dimY / 2.
 * box: DEVICE [n][4] int32 (row0, row1, col0, col1), half-open, outside of which slice z holds only label 0 (row1 <= row0:
 * an empty slice), or NULL.  It only spares steps whose four labels are empty: exact zeros.
 * Limits: 1 <= m <= 8192, 1 <= n <= 65535, 1 <= nmat <= PSX_VOLUME_MAX_MAT, 1 <= dimY <= 2^20, 1 <= dimX <= 2^24,
 * nmat*dimX*dimY <= 2^40, s finite in [1/64, 64], voxel_m finite. */
#define PSX_VOLUME_MAX_MAT 16
typedef struct {
    int n, m, nmat;
    int dimX, dimY;
    double cos_a, sin_a, off_x, off_y;   /* radon's inverse map about c = m / 2 */
    double s;                            /* study pixel / voxel */
    double voxel_m;
    const int32_t *box;                  /* DEVICE [n][4], or NULL */
} psx_volume_desc;
int psx_volume_project_u8(const psx_volume_desc *desc, const uint8_t *labels, double *lines_or_null, float *geom, void *stream);

/* ---- the same volume under a point source: divergent (cone-beam) projection -----------------------------------------------
 * Geometry, in voxels about the rotation axis: depth w = r - c0 along the walk (c0 = m / 2, the walk ascending in r), t
 * across the axis, z the height above the optical axis.  The source is at (t, w, z) = (0, -dso, 0); the study grid is the
 * virtual detector through the axis, the plane w = 0, so a ray through its point (t0, z0) is at (t0 g, z0 g) at depth w,
 * g = (dso + w)/dso.  Same descriptor, buffers and limits as psx_volume_project_u8, plus dso in [m, 1e30] (PSX_E_ARG
 * otherwise, NaN included): the source lies outside the slice's bounding circle and dso + w > 0 on the whole walk.
 * In float64, every product, quotient, sum and square root rounded on its own (no contraction), for study pixel (x, y):
 *   t0 = (double)(y - dimY / 2) * s,  z0 = (double)(x - dimX / 2) * s;  for r = 0 .. m - 1 in ascending order
 *   g = (dso + (double)(r - c0)) / dso;  cpos = t0 * g + (double)c0;  slice z = n / 2 + (int)floor(z0 * g + 0.5), and a step
 *   whose z is outside [0, n) adds nothing;  X = cos*cpos + sin*r + off_x,  Y = (-sin*cpos) + cos*r + off_y, and the floors,
 *   the ceils, dr, dc and the bilinear indicator term of material k are psx_volume_project_u8's, on slice z:  acc_k += term.
 *   L = sqrt(1 + (t0*t0 + z0*z0)/(dso*dso)), the path length of a unit step in w;
 *   lines[k][x][y] = acc_k * L,  geom[k][x][y] = (float)(lines[k][x][y] * voxel_m).
 * No atomics and no reduction across lanes: the order above is the order of the sum.  box spares steps as above.  At
 * dso >= 2^66 every g is exactly 1 and L is 1: the maps are psx_volume_project_u8's bit for bit. */
int psx_volume_project_cone_u8(const psx_volume_desc *desc, double dso, const uint8_t *labels, double *lines_or_null,
                               float *geom, void *stream);

/* ---- phase retrieval of speckle image stacks (no counterpart in the reference: its images' consumer) -----------------
 * LCS ("Low Coherence System", Quenot et al., Optica 8, 1412, 2021) over K positions of one energy bin: per pixel,
 *   R_k ~ x0*S_k + x1*g0_k + x2*g1_k,  (g0, g1) = np.gradient(R_k) (unit spacing, edge_order=1, float32 differences),
 *   M = sum_k a_k a_k^T and v = sum_k a_k R_k with a_k = (S_k, g0_k, g1_k) in float64, M x = v solved in float64;
 *   x = (1, 0, 0) exactly when det M <= 1e-12*M00*M11*M22 or the solved x0 <= 0 (or is not a finite number);
 *   transmission = 1/x0, dx = x1 (axis 0), dy = x2 (axis 1), detector pixels, the sign of the chain's Dxreal / Dyreal;
 *   max_shift > 0 clamps dx, dy into [-max_shift, max_shift] (0: no clamp).
 *   Non-finite input (psx_lcs_df_f32 too): a pixel reads its own S_k and R_k and the four neighbours of R_k at the clamped
 *   indices; if one of these samples is NaN or +-inf for some k, the pixel returns the fallback, (1, 0, 0) or (1, 0, 0, 0).
 *   Every other pixel is untouched: it has the bits it has on finite images.
 * S, R: HOST arrays of K in [3, PSX_MAX_LCS] device pointers to n x m float32 images (n, m >= 3); one launch reads each
 * image once.  transmission, dx, dy: n x m float32, written. */
#define PSX_MAX_LCS 64
int psx_lcs_f32(const float *const *S, const float *const *R, int K, int n, int m, float max_shift, float *transmission,
                float *dx, float *dy, void *stream);
/* LCS-DF: psx_lcs_f32 with a dark-field column (the diffusion term of the X-ray Fokker-Planck model, Morgan & Paganin,
 * Sci. Rep. 9, 17465, 2019): per pixel, R_k ~ x0*S_k + x1*g0_k + x2*g1_k + x3*L_k, L_k = R[i+1,j] + R[i-1,j] + R[i,j+1] +
 *   R[i,j-1] - 4 R[i,j] with edge-replicated neighbours (the gradients' clamped indices), formed in float64;
 *   M (4x4), v as above with a_k = (S_k, g0_k, g1_k, L_k), solved by LDL^T without pivoting in float64;
 *   x = (1, 0, 0, 0) exactly when a pivot d_i <= 0, prod d_i <= 1e-12*M00*M11*M22*M33, or the solved x0 <= 0;
 *   transmission = 1/x0, dx = x1, dy = x2 as psx_lcs_f32 (max_shift clamps these two only), df = -x3 in detector px^2
 *   (S ~ T*(R - D.grad R + df*lap R); a Gaussian blur of per-axis variance s^2 gives df = s^2/2), not clamped.
 * K in [4, PSX_MAX_LCS], n, m >= 3; argument errors as psx_lcs_f32.  Reads the same bytes as psx_lcs_f32, writes four maps. */
int psx_lcs_df_f32(const float *const *S, const float *const *R, int K, int n, int m, float max_shift, float *transmission,
                   float *dx, float *dy, float *df, void *stream);
/* UMPA ("Unified Modulated Pattern Analysis", Zdora et al., PRL 118, 203903, 2017; separable form: De Marco et al., Opt.
 * Express 31, 635, 2023): windowed speckle tracking for displacements beyond the one pixel LCS is valid for, from K >= 1
 * positions.  Model S_k(q) ~ T*R_k(q - u), LCS's sign: dx along axis 0, dy along axis 1, as the chain's Dxreal / Dyreal.
 *   window = w in [1, PSX_MAX_UMPA_WINDOW]: a UNIFORM (2w+1)^2 window (no Hamming taper, unlike the UMPA package: the window
 *   sums are then box filters); search = s in [1, PSX_MAX_UMPA_SEARCH]: integer candidates u = (a, b), |a|, |b| <= s;
 *   K in [1, PSX_MAX_LCS]; n, m >= 2(w+s)+1.
 *   Border band: a pixel closer than w+s to any border gets exactly transmission = 1, dx = dy = 0, residual = 0; no index is
 *   ever clamped or mirrored.
 *   Interior pixel r, sums over k and over q in the window around r, all in float64 (any order):
 *     E = sum S_k(q)^2,  B(u) = sum S_k(q) R_k(q-u),  C(u) = sum R_k(q-u)^2;  a candidate with C(u) == 0 is skipped;
 *     L(u) = E - B*B/C,  T(u) = B/C;  u* = (a*, b*) = the first strict minimum of L, a outer, b inner, both ascending;
 *     per axis: if |a*| < s and both L(a*-1, b*) = Lm and L(a*+1, b*) = Lp exist (not skipped), den = Lm - 2 L(u*) + Lp and,
 *     if den > 0, da = clip(0.5 (Lm - Lp)/den, -0.5, 0.5); otherwise da = 0 (a minimum on the search boundary gives
 *     exactly +-s); db likewise;
 *     dx = a* + da, dy = b* + db, transmission = T(u*), residual = max(L(u*), 0)/E, as float32;
 *     (1, 0, 0, residual 0) exactly when every candidate is skipped or T(u*) <= 0.
 *   Where two candidates' costs agree to rounding the choice between them is unspecified.
 * S, R: HOST arrays of K device pointers to n x m float32 images, n*m <= 2^30.  One launch, no scratch memory: the images
 * are read (2s+1)*ceil((2s+1)/7) times from L2 at most.  Argument errors as psx_lcs_f32. */
#define PSX_MAX_UMPA_WINDOW 8
#define PSX_MAX_UMPA_SEARCH 8
int psx_umpa_f32(const float *const *S, const float *const *R, int K, int n, int m, int window, int search,
                 float *transmission, float *dx, float *dy, float *residual, void *stream);
/* UMPA with its dark-field (visibility) term, the third modality of Zdora et al.: psx_umpa_f32 with the model
 *   S_k(q) ~ alpha*R_k(q - u) + beta*mu_k = T*[mu_k + V*(R_k(q - u) - mu_k)],  T = alpha + beta,  V = alpha/T,
 * mu_k the mean intensity of reference frame k: a sample that blurs the speckle lowers their visibility by V < 1.
 *   mean: HOST array of K finite float64 values mu_k (copied into the argument block).
 *   K, window = w, search = s, the image sizes, the border band, the candidate order, "first strict minimum", the parabola
 *   and the argument errors are psx_umpa_f32's, word for word.
 *   Interior pixel r, sums over k and over q in the window around r, all in float64 (any order): E, B(u), C(u) as
 *   psx_umpa_f32, and
 *     F = sum mu_k S_k(q),  G(u) = sum mu_k R_k(q-u),  H = (2w+1)^2 sum_k mu_k^2.
 *   Then, each ONE rounded IEEE operation (no contraction into fma anywhere in the sequence):
 *     p = C*H;  q = G*G;  det = p - q;  the candidate is skipped unless det > 1e-12*p (which covers C == 0, H == 0 and a
 *     reference window proportional to mu);
 *     alpha = (B*H - F*G)/det;  beta = (C*F - G*B)/det;  L = E - (alpha*B + beta*F);  T = alpha + beta;
 *     u*, da, db exactly as psx_umpa_f32, on this L;
 *     transmission = T(u*), visibility = alpha(u*)/T(u*), residual = max(L(u*), 0)/E, dx, dy as psx_umpa_f32, as float32;
 *     (1, 0, 0, visibility 1, residual 0) exactly when every candidate is skipped or T(u*) <= 0, and in the border band.
 *   visibility is not clamped: noise and model error give values above 1 or below 0, which are returned as they are.
 * One launch, no scratch memory, the image traffic of psx_umpa_f32. */
int psx_umpa_df_f32(const float *const *S, const float *const *R, const double *mean, int K, int n, int m, int window,
                    int search, float *transmission, float *dx, float *dy, float *visibility, float *residual, void *stream);
/* Frankot-Chellappa integration (IEEE PAMI 10, 1988) of the gradient field scale*(gx, gy) (rad per pixel along axis 0 / 1)
 * with mirror extension: on the 2n x 2m grid gx is odd in axis 0 and even in axis 1, gy even in axis 0 and odd in axis 1;
 * P = (-i kx Gx^ - i ky Gy^)/(kx^2 + ky^2), P(0) = 0, kx = 2 pi fftfreq(2n), ky = 2 pi fftfreq(2m); phi = Re ifft2(P) on
 * the n x m corner (zero mean over the extension).  Both gradients go through ONE complex transform pair (Z = Gx + i Gy,
 * rocFFT single precision, in place).  A plan fixes n x m and owns the 2n x 2m complex64 buffer and rocFFT's work
 * buffer; psx_integrate_plan_bytes reports them.  gx, gy, phi: n x m float32 device images. */
int psx_integrate_plan_create(int n, int m, psx_integrate_plan **plan);
int psx_integrate_plan_destroy(psx_integrate_plan *plan);
size_t psx_integrate_plan_bytes(const psx_integrate_plan *plan);
int psx_integrate_f32(psx_integrate_plan *plan, const float *gx, const float *gy, double scale, float *phi, void *stream);
/* Paganin's single-distance, single-material phase retrieval (Paganin et al., J. Microsc. 206, 33, 2002) of B propagation
 * images of the plan's n x m shape, on the plan's 2n x 2m buffer and transforms (no allocation in the call).  Per image b,
 * I = image[b], I0 = white[b] (the flat field; absent when `white` or white[b] is NULL), alpha[b] >= 0 the filter strength
 * in detector px^2, mu[b] > 0 the linear attenuation coefficient in 1/m (both HOST arrays of B finite values):
 *   r = I/I0 formed in float64 (r = I where I0 is absent); a pixel whose I is not finite, or whose I0 is not finite or
 *   not > 0, gets r = 1;
 *   x = float32(r - 1): the transform carries r - 1, not r (the filter passes DC unchanged, and the float32 transform
 *   error then scales with the contrast, not with 1);
 *   ext[a][b] = x[a < n ? a : 2n-1-a][b < m ? b : 2m-1-b], the even mirror extension, psx_integrate_f32's indices;
 *   y = ifft2( fft2(ext) / (1 + alpha*(kx^2 + ky^2)) ), kx = 2 pi fftfreq(2n), ky = 2 pi fftfreq(2m) (psx_integrate_f32's),
 *   the denominator formed in float64;
 *   c = 1 + y on the n x m corner: the contact image exp(-mu*t);
 *   thickness = -log1p(y)/mu in float64 where c > 0, else -log(FLT_MIN)/mu: finite wherever y is.
 * Two images share one complex transform pair: image 2j is the real part, image 2j+1 the imaginary part (zero for a last
 * odd image); the filter separates the two spectra through the Hermitian pair (k, -k), A^(k) = (Z(k) + conj Z(-k))/2,
 * B^(k) = (Z(k) - conj Z(-k))/(2i), applies each image's own factor and recombines A^ + i B^; self-paired points (DC, the
 * Nyquist row and column) go through the same formula.
 * image: HOST array of B in [1, PSX_MAX_PAGANIN] device pointers to n x m float32 images.  contact, thickness: HOST arrays
 * of B device pointers to n x m float32 outputs; either array, or single entries of it, may be NULL (that map is not
 * written), but every image needs one of the two.  Calls on one plan (psx_integrate_f32's included) are ordered on one
 * stream: they share its buffer. */
#define PSX_MAX_PAGANIN 64
int psx_paganin_f32(psx_integrate_plan *plan, int B, const float *const *image, const float *const *white,
                    const double *alpha, const double *mu, float *const *contact, float *const *thickness, void *stream);

/* ---- filtered back-projection (parallel beam) of a stack of projections: sinogram -> volume ----------------------------
 * sino [A][n][m] float32: A projections, each an n x m map; axis 0 (n) runs along the rotation axis, so detector row r of all
 * projections is one slice, axis 1 (m) across it.  theta: HOST array of A finite angles in degrees (any values: negative,
 * >= 180, repeated); center: the detector column of the rotation axis (m / 2 rounded down is skimage radon's).
 * vol [n][m][m] float32, vol[r][i][j]: slice row i, slice column j, the orientation of the slice radon projects.
 * Filter, per line sino[a][r][:], P = max(64, 2^ceil(log2(2m))):
 *   f[0] = 1/4, f[j] = -1/(pi*jj)^2 for odd jj = min(j, P - j), 0 otherwise;  H = 2*Re FFT_P(f), formed in float64 on the host;
 *   PSX_FBP_HANN multiplies H by fftshift(hanning(P)), hanning(P)[n] = 0.5 - 0.5*cos(2 pi n/(P-1)); PSX_FBP_NONE: H = 1;
 *   q = Re IFFT_P( FFT_P(line zero-padded to P) * H )[:m].  Two lines share one complex transform (rocFFT, single
 *   precision): the real part of the filtered pair is that of a filter with the even part (H[k] + H[P-k])/2, which is what
 *   the device multiplies by, so the two lines do not mix.  PSX_FBP_NONE copies the lines and runs no transform.
 * Differential filters (PSX_FBP_DIFFERENTIAL set): the line holds d(sinogram)/d(column), per detector pixel -- what
 *   differential phase contrast (speckle tracking, gratings) measures.  The ramp is the derivative followed by a Hilbert
 *   transform, 2|f| = (i 2 pi f) * (-i sgn f / pi), so such a line takes the Hilbert filter alone:
 *   g[j] = 2/(pi^2 s) for odd signed lag s (s = j for j < P/2, s = j - P for j > P/2), 0 for even s and at j = P/2;
 *   G = FFT_P(g), formed in float64 on the host, is purely imaginary and odd; Ho = Im G with Ho[0] = Ho[P/2] = 0 exactly;
 *   PSX_FBP_HILBERT_HANN multiplies Ho by the window of PSX_FBP_HANN;
 *   q = Re IFFT_P( FFT_P(line zero-padded to P) * i*Ho )[:m], i.e. q[k] = sum_j g[k - j]*line[j].  The real part is that of
 *   the filter with the odd part (Ho[k] - Ho[P-k])/2, which is Hermitian as i*Ho: the device multiplies the pair's
 *   transform Z by it, Z <- (-Z.y*w, Z.x*w) with w the odd part over P in float64, and the two lines do not mix.
 *   Every lag |k - j| < m <= P/2 is inside the kernel, so the convolution of a line that vanishes off the detector is
 *   linear, not wrapped.  Ho[0] = 0 removes a constant offset of the padded line, not of the line: an offset c on the m
 *   samples is a box, whose Hilbert transform grows towards its ends -- it is NOT removed exactly (an offset of 1 % of the
 *   largest |dp/du| moves the three-blob volume of tests/_hilbert_oracle.py by up to 1.0 % of its peak at m = 64).
 *   Back-projection and the pi/(2A) scale are the ramp's: with this sign psx_fbp_f32 on dp/du (u the column index)
 *   reproduces PSX_FBP_RAMP on p, to discretisation.
 * Back-projection, h = m / 2 rounded down, c_a = cos(theta_a*pi/180), s_a = sin(theta_a*pi/180) in float64 on the host:
 *   u = (j - h)*c_a - (i - h)*s_a + center in float64;  q(u) by linear interpolation between the samples with
 *   q[-1] = q[m] = 0, and 0 for u <= -1 or u >= m (continuous in u, unlike np.interp(left=0, right=0));
 *   vol[r][i][j] = pi/(2A) * sum_a q_{a,r}(u), accumulated in float32 in ascending a;
 *   circle != 0: voxels with (i - h)^2 + (j - h)^2 > h^2 are 0.
 * A plan fixes (A, m, theta, center, filter, circle) and owns the tables, the transform and the filtered sinogram of
 * max_rows detector rows (0: as many as fit 256 MiB, at least 2, at most 64; otherwise rounded up to an even count):
 * psx_fbp_f32 walks the n rows in blocks of that many, so the work buffer is bounded whatever n is;
 * psx_fbp_plan_bytes reports it with rocFFT's.  A in [1, PSX_FBP_MAX_ANGLES], m in [2, PSX_FBP_MAX_M], n >= 1,
 * |center| <= 2^20.  Calls on one plan are ordered on one stream: they share its buffer. */
#define PSX_FBP_RAMP 0
#define PSX_FBP_HANN 1
#define PSX_FBP_NONE 2
#define PSX_FBP_DIFFERENTIAL 16            /* the line holds d(sinogram)/d(column), per pixel */
#define PSX_FBP_HILBERT      (PSX_FBP_DIFFERENTIAL | PSX_FBP_RAMP)   /* 16 */
#define PSX_FBP_HILBERT_HANN (PSX_FBP_DIFFERENTIAL | PSX_FBP_HANN)   /* 17 */
#define PSX_FBP_MAX_ANGLES 4096
#define PSX_FBP_MAX_M 8192
typedef struct psx_fbp_plan psx_fbp_plan;
int psx_fbp_plan_create(int A, int m, const double *theta_deg, double center, int filter, int circle, int max_rows,
                        psx_fbp_plan **plan);
int psx_fbp_plan_destroy(psx_fbp_plan *plan);
size_t psx_fbp_plan_bytes(const psx_fbp_plan *plan);
int psx_fbp_f32(psx_fbp_plan *plan, const float *sino, int n, float *vol, void *stream);

/* ---- the matched projector pair of a plan: B (back-projection without filter and scale) and its transpose ---------------
 * B is the interpolation operator of the back-projection above, per angle a and voxel (i, j):
 *   u = fma(j - h, c_a, fma(-(i - h), s_a, center)) in float64;  fl = floor(u);  w1 = (float)(u - fl);  w0 = 1.0f - w1;
 *   (B q)[r][i][j] = sum_a w0*q[a][r][fl] + w1*q[a][r][fl + 1], q[-1] = q[m] = 0, in float32 in ascending a;
 *   circle != 0: (B q) is 0 on the voxels with (i - h)^2 + (j - h)^2 > h^2.
 * psx_fbp_adjoint_f32: vol [n][m][m] = B sino, sino [A][n][m]: unfiltered and with scale 1 on any plan (the plan's filter
 *   is ignored); it uses the plan's buffer in the row blocks of psx_fbp_f32.  On a PSX_FBP_NONE plan psx_fbp_f32 is
 *   float32(pi/(2A)) times it, bit for bit.
 * psx_fbp_project_f32: sino [A][n][m] = B^T vol, vol [n][m][m], the exact transpose:
 *   sino[a][r][k] = sum over the voxels (i, j) (the lit ones when circle != 0) of t*vol[r][i][j],
 *   t = w0 if k == fl, w1 if k == fl + 1, else 0: the weights are bit for bit B's, never formed from an inverted
 *   coordinate.  Unscaled: a line integral in pixels, the unit psx_fbp_f32 consumes.  The plan's filter is ignored.
 *   Summation order, float32 fused multiply-adds: the slice is walked in lines of its major axis -- lines of constant i
 *   when |c_a| >= |s_a|, of constant j otherwise -- line L goes to partial sum L & 3, each partial takes its lines in
 *   ascending L and the voxels of a line in ascending minor index, and the sample is (p0 + p1) + (p2 + p3).  No atomics:
 *   two calls return the same bits, whatever n and the plan's max_rows are.
 * Both refuse a null plan, null pointers and n < 1, and are asynchronous on the stream. */
int psx_fbp_project_f32(psx_fbp_plan *plan, const float *vol, int n, float *sino, void *stream);
int psx_fbp_adjoint_f32(psx_fbp_plan *plan, const float *sino, int n, float *vol, void *stream);

/* ---- the voxel step of total-variation reconstruction on the pair ------------------------------------------------------
 * min 0.5*|B^T x - b|^2 + lambda*TV(x) per detector row by the primal-dual hybrid gradient method with Pock and
 * Chambolle's diagonal preconditioners (alpha = 1): TV the isotropic total variation of the slice by forward differences.
 * The caller projects (q = B^T xbar), updates the data dual y and back-projects it (u = B y); this call does the rest of an
 * iteration for the n slices in one launch.  With lit(i, j) the plan's circle mask (every voxel of the slice without
 * circle), ax(i, j) = lit(i, j) and lit(i + 1, j) (i + 1 < m) the active difference along i, ay(i, j) along j, and
 * deg(i, j) = ax(i, j) + ax(i - 1, j) + ay(i, j) + ay(i, j - 1), per voxel in float32:
 *   gx = ax ? xbar[i+1][j] - xbar[i][j] : 0, gy likewise;  tx = fma(0.5, gx, px), ty = fma(0.5, gy, py);
 *   nr = sqrt(fma(tx, tx, ty*ty));  (px', py') = nr > lambda ? (tx*s, ty*s), s = lambda/nr : (tx, ty);
 *   d = ((ax(i-1,j) ? px'[i-1][j] : 0) - (ax(i,j) ? px'[i][j] : 0) + (ay(i,j-1) ? py'[i][j-1] : 0)) - (ay(i,j) ? py'[i][j] : 0);
 *   tau = c + deg > 1e-6 ? 1/(c + deg) : 0;  x' = fma(-tau, u + d, x), then max(x', 0) if nonneg;  xbar' = fma(2, x', -x).
 * u, c (= B 1), x, xbar, px, py are [n][m][m]; x is updated in place, xbar and p go from their _in to their _out buffers
 * (a tile reads its neighbours' xbar and forms their p' again, the same bits), which the caller swaps.  lambda is rounded
 * to float32; with lambda = 0 the dual comes out exactly 0.  No atomics: the same input gives the same bits, and a slice
 * gives the bits it gives alone.  PSX_E_ARG, before any launch: a null plan or pointer, n < 1, lambda negative or not
 * finite, xbar_out == xbar_in, px_out == px_in, py_out == py_in, xbar_out == x.  Asynchronous on the stream. */
int psx_fbp_tv_step_f32(psx_fbp_plan *plan, int n, double lambda, int nonneg, const float *u, const float *c, float *x,
                        const float *xbar_in, float *xbar_out, const float *px_in, const float *py_in, float *px_out,
                        float *py_out, void *stream);

/* ---- FDK: filtered back-projection of a full-turn cone-beam scan (Feldkamp, Davis, Kress, JOSA A 1, 612, 1984) ------------
 * sino [A][n][m] float32 on the virtual detector through the rotation axis (pixel = voxel), as psx_fbp_f32's; theta: A
 * angles in degrees, meant to cover a full turn evenly; center: the axis's column; vcenter: the optical axis's row (a
 * double: fractional, or outside [0, n)); dso: the source's distance from the axis in voxels, in [m, 1e30]; filter:
 * PSX_FBP_RAMP, _HANN or _NONE (the differential filters are refused).  vol [n][m][m]; slice Z lies at height Z - vcenter.
 * The geometry is psx_volume_project_cone_u8's: at angle a, voxel (i, j), h = m / 2, has t = (j - h) c_a - (i - h) s_a across
 * the axis and the depth w = (j - h) s_a + (i - h) c_a, and is seen at (t U, z U), U = dso/(dso + w).
 *   1. Pre-weight, in float64, each operation rounded on its own, fused into the pack:  dk = (double)k - center,
 *      dr = (double)r - vcenter,  p' = (float)((double)p * dso / sqrt((dso*dso + dk*dk) + dr*dr)).
 *   2. The lines of p' are filtered exactly as psx_fbp_f32 filters them (the same H, two lines per transform, the same code).
 *   3. Back-projection, per angle and voxel in float64, each operation rounded on its own (no contraction):
 *      t = dj*c - di*s,  w = dj*s + di*c  (dj = j - h, di = i - h);  U = dso/(dso + w);  u = t*U + center;
 *      v = ((double)Z - vcenter)*U + vcenter.  The sample is bilinear in (v, u) with the float32 weights of B:
 *      fl = floor(coord), w1 = (float)(coord - fl), w0 = 1.0f - w1, on q with q[-1][.] = q[n][.] = q[.][-1] = q[.][m] = 0,
 *      and 0 unless -1 < u < m and -1 < v < n: continuous at the detector's edges in both axes.  In float32:
 *      lo = fmaf(wu1, q[fv][fu+1], wu0*q[fv][fu]),  hi = fmaf(wu1, q[fv+1][fu+1], wu0*q[fv+1][fu]),
 *      acc = fmaf((float)(U*U), fmaf(wv1, hi, wv0*lo), acc) in ascending a;  vol[Z][i][j] = acc * (float)(pi/(2A)).
 *      circle != 0: voxels with (i - h)^2 + (j - h)^2 > h^2 are 0.
 * The scale is the ramp's own: H is 2|f|, and FDK over a full turn is (1/2) int_0^2pi U^2 (p' * |f|) dbeta = (pi/A) sum, hence
 * pi/(2A) sum with this filter.  As dso grows the volume tends to psx_fbp_f32's.
 * A voxel of slice Z reads detector rows other than Z, so the plan fixes n as well and owns the filtered sinogram of all
 * rows, A*n*m float32, besides a parallel plan's tables, transforms and row-block buffer; psx_fdk_plan_bytes reports both.
 * PSX_E_ARG: A*n*m above PSX_FDK_MAX_SAMPLES (2^31 samples, 8 GiB), n outside [1, 65535], |vcenter| > 2^20, dso outside
 * [m, 1e30] or NaN, a differential filter, and whatever psx_fbp_plan_create refuses.  Deterministic, no atomics: a voxel's
 * bits do not depend on n's blocks.  Calls on one plan are ordered on one stream. */
#define PSX_FDK_MAX_SAMPLES ((int64_t)1 << 31)
typedef struct psx_fdk_plan psx_fdk_plan;
int psx_fdk_plan_create(int A, int n, int m, const double *theta_deg, double center, double vcenter, double dso, int filter,
                        int circle, psx_fdk_plan **plan);
int psx_fdk_plan_destroy(psx_fdk_plan *plan);
size_t psx_fdk_plan_bytes(const psx_fdk_plan *plan);
int psx_fdk_f32(psx_fdk_plan *plan, const float *sino, float *vol, void *stream);

/* ---- spectral material decomposition of energy-binned scans (paresis_amd/spectral.py) -------------------------------------
 * Projection-domain decomposition: per pixel, from the B per-bin log-transmissions L_b = -ln(transmission of bin b), the
 * thicknesses x_m (metres) of M <= B materials under the polychromatic model
 *   T_b(x) = sum_e w_be exp(-sum_m a_mbe x_m),
 * w_be the flat field's per-energy share of bin b (each bin's summing to 1), a_mbe the linear attenuation coefficient of
 * material m at that energy (1/m): beam hardening is part of the model.  Per pixel, in float64 throughout:
 *   any L_b not finite: thickness 0, residual +inf, steps -1;
 *   start x = G L, G the M x B matrix of the linearised problem, (Abar^T V Abar)^-1 Abar^T V with Abar_bm = sum_e w_be a_mbe
 *   (the caller's: row-major [M][B]);
 *   iteration k = 1 .. iterations (weighted Gauss-Newton): per bin s_e = w_be exp(-sum_m a_mbe x_m), T_b = sum_e s_e,
 *   g_bm = sum_e a_mbe s_e / T_b, r_b = L_b + ln T_b; N = sum_b v_b g_b g_b^T and rhs = sum_b v_b g_b r_b are added to bin by
 *   bin; N d = rhs by LDL^T without pivoting (as psx_lcs_df_f32).  A pivot <= 0 or not finite, or a d that is not finite:
 *   steps = -2 and x is kept.  Otherwise x += d, steps = k, and the pixel stops when max_m |d_m| abar_m <= tol,
 *   abar_m = max_b Abar_bm: on its own step alone, so a pixel's result does not depend on its neighbours;
 *   residual = sqrt(sum_b v_b r_b^2) at the final x.  The thickness is never clamped.
 * A pixel with L = 0 in all bins gives exactly 0 where every bin's weights sum to exactly 1 in float64.
 * logT: HOST array of B device pointers to n float32 values; bin_size[b] >= 1 energies in bin b, their sum E <= 256; w: the E
 * weights, bin after bin; a: [M][E]; v: B bin weights, each finite and > 0; G: [M][B] -- HOST arrays all, copied in the
 * call.  thickness: HOST array of M device pointers to n float32 values; residual, steps: n float32 each, or NULL.
 * PSX_E_ARG, before any GPU call: a null pointer, B outside [1, PSX_DECOMP_MAX_BINS], M outside [1, PSX_DECOMP_MAX_MAT],
 * M > B, a bin size < 1 or a sum above PSX_DECOMP_MAX_ENERGIES, a v that is not finite and > 0, iterations < 1, tol negative or
 * not finite, n < 1.  One launch; like psx_membrane_f32 the call waits for the stream once (the tables' upload). */
#define PSX_DECOMP_MAX_MAT 4
#define PSX_DECOMP_MAX_BINS 8
#define PSX_DECOMP_MAX_ENERGIES 256      /* all bins together */
int psx_decompose_f32(const float *const *logT, int B, const int *bin_size, const double *w, const double *a, int M,
                      const double *v, const double *G, int iterations, double tol, int64_t n,
                      float *const *thickness, float *residual, float *steps, void *stream);

/* ---- per-kernel timing (bench.py's roofline leg) ----------------------------------------------------------------------
 * psx_profile_enable(1) clears the log and makes every kernel launch of the library record a HIP event pair on the
 * stream it is launched on; psx_profile_summary() waits for the recorded events and writes one line per kernel,
 * "name count total_ms\n".  Off by default (no events, no overhead). */
int psx_profile_enable(int on);
int psx_profile_summary(char *buf, size_t cap);

/* Diagnostics: device buffer receiving phase timestamps (100 MHz wall clock): 32 x uint64 per workgroup from the line
 * kernels of the LDS Fresnel engine, 16 x uint64 per workgroup from the refraction kernel (tools/stamp_*.py).
 * NULL (default) switches it off.  Never enabled in timed runs. */
int psx_debug_stamps(void *buf);

/* Diagnostic A/B switches, process-wide, all off by default; the library reads NOTHING from the environment.  Names:
 *   "stamp_pass1", "stamp_round" (default 1), "detect_4pass", "no_p2" (read when a Fresnel plan is created: the
 *   576*R3-point line transforms of round 5 instead of the power-of-two ones).  tools/ and tests/ set them; timed product runs never do.  psx_debug_switches_active writes
 *   "name=value ..." of every switch that is not at its default (empty string: none) -- bench.py echoes it in its JSON line. */
int psx_debug_switch(const char *name, int value);
int psx_debug_switches_active(char *buf, size_t cap);

/* ---- status word ------------------------------------------------------------------------------------------------ */
/* OR PSX_STATUS_NONFINITE into *status when img holds NaN or |v| > 1e50 (float32: inf) */
int psx_status_scan_f32(const float *img, int64_t n, unsigned *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PARESIS_HIP_H */
