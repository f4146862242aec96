/*
 * ife_hip.h -- C-ABI of the MI355X (gfx950) per-voxel Hessian feature engine.
 *
 * This is the drop-in boundary for the hot path of orting/image-feature-extraction:
 * the reference runs the path as ITK filter objects inside one process
 * (headers under include/ife/Filters and include/ife/Numerics); here every stage that the
 * reference exposes as a filter / functor / tool body has one extern "C" entry
 * point taking plain pointers and sizes.  The C++ host classes under
 * image-feature-extraction_amd/host/ (same class and method names as the
 * reference) and the tools forward to these entry points; INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - volumes are x-fastest: index = x + nx*(y + ny*z)  (itk::Image buffer order)
 *   - vector outputs: IFE_INTERLEAVED [voxel*ncomp + c] (itk::VectorImage order) or
 *     IFE_PLANAR [c*nvox + voxel]
 *   - IFE_MEM_HOST: pointers are host memory, the call copies in/out and blocks;
 *     IFE_MEM_DEVICE: pointers are device (HBM) memory on the context's device, the
 *     call enqueues on the context's stream and returns without synchronising
 *   - every call returns 0 or a negative ife_status; ife_last_error() gives text
 *   - an ife_ctx is single-owner (one host thread at a time); different contexts
 *     may run concurrently
 *   - there is no CPU fallback: every entry point fails with IFE_E_HIP when no
 *     gfx950 device is usable
 *
 * All "reference" citations are paths relative to the reference repository root.
 */
#ifndef IFE_HIP_H
#define IFE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IFE_ABI_VERSION 1

typedef struct ife_ctx ife_ctx;

typedef enum {
  IFE_OK = 0,
  IFE_E_ARG = -1,    /* null pointer, bad enum, bad sigma/spacing */
  IFE_E_SIZE = -2,   /* an axis shorter than 4 where the recursive Gaussian runs
                        (ITK throws for ln < 4), or a non-positive size */
  IFE_E_HIP = -3,    /* HIP runtime error (text in ife_last_error) */
  IFE_E_NOMEM = -4,  /* device or host allocation failed */
  IFE_E_STATE = -5   /* call sequence error (slab API) */
} ife_status;

typedef enum { IFE_F32 = 0, IFE_I16 = 1, IFE_U8 = 2, IFE_U16 = 3 } ife_dtype;
typedef enum { IFE_INTERLEAVED = 0, IFE_PLANAR = 1 } ife_layout;
typedef enum { IFE_MEM_HOST = 0, IFE_MEM_DEVICE = 1 } ife_mem;
/* IFE_MEM_DEVICE pointers must be aligned to their element size, interleaved 8-component
 * outputs to 16 bytes, 6- and 10-component ones to 8 (vector stores); anything else is refused
 * with IFE_E_ARG.  hipMalloc'ed buffers and whole voxels / planes inside them qualify. */

/* Options for ife_ctx_set_option */
typedef enum {
  /* How the solver's unqualified sqrt/acos/cos (Symmetric3x3EigenvalueSolver.h:88,115,
   * 119-120) are evaluated.  0: in double, the binding the reference gets when only <cmath>
   * is visible (bit-identical to a libm build except at about one voxel in 10^8);
   * 1: float overloads (<math.h> visible), correctly rounded;
   * 2 (default): q, p, B and r as in 0/1, acos and cos by float polynomials: eigenvalues
   * within 1e-6 |lambda_1| of mode 0 (measured maximum in DESIGN.md; the contract of this
   * library is 1e-5), the spread the reference itself has between contexts 0 and 1, at a
   * fifth of the instructions.  Two eigenvalues whose magnitudes tie within that error may
   * come out in the other order.  The environment variable IFE_TRIG_MODE=0|1|2 sets the
   * initial value at ife_ctx_create (for the tools, which have no flag for it). */
  IFE_OPT_TRIG_MODE = 1,
  /* 0 (default): DerivativeImageFilter scales by 1/spacing once whatever the order
   * (upstream ITK behaviour); 1: 1/spacing^order.  Same for unit spacing. */
  IFE_OPT_DSCALE_MODE = 2,
  /* 1: record a hipEvent pair around every kernel launch so that
   * ife_get_kernel_times can report per-kernel device time.  Default 0. */
  IFE_OPT_PROFILE = 3,
  /* planes per workgroup march of the feature kernel (default 64) */
  IFE_OPT_ZCHUNK = 4,
  /* samples per register block of the recursive-Gaussian kernels: 0 (default: chosen per
   * axis -- z 12, y 12, x 16), or 8, 10, 12, 16 for both strided axes
   * (x keeps 16 unless 8 is asked for).  Never changes results. */
  IFE_OPT_IIR_BLOCK = 5,
  /* register blocks per checkpoint of the strided (z, y) line kernel: 2 (default, measured
   * faster) or 1 */
  IFE_OPT_IIR_CKPT = 6,
  /* 1: fuse each multiply-add of the recursive Gaussian (half the double operations).  Not
   * the reference's arithmetic: outputs differ by one float ulp at about one voxel in 10^8,
   * which the second differences can amplify past the 1e-5 bar there.  Default 0. */
  IFE_OPT_IIR_FMA = 7,
  /* 1 (default): the last axis pass of the normalized convolution runs numerator and
   * denominator in sibling waves and stores only their quotient (the Div functor,
   * NormalizedGaussianConvolutionImageFilter.hxx:57-61); 0: two float fields and a division
   * in the consumer.  Same results bit for bit. */
  IFE_OPT_FUSED_DIVIDE = 8,
  /* 1 (default): a line of the recursive Gaussian whose samples all have one bit pattern --
   * +0, -0 (T * 0 where T < 0) or 1.0f -- is answered with the constant the filter makes of
   * it, where the host has established that constant by running this sigma and line length
   * through the kernels' arithmetic (decided per wave of 64 adjacent lines): the exterior of a
   * mask costs a read and a write.  Same results bit for bit, signs of zero included; 0:
   * every line is filtered. */
  IFE_OPT_CONST_LINES = 9,
  /* 1 (default): where the feature kernel reads ONE float field (the smoothed value after a
   * quotient-storing last pass, or a raw float image) and the mask is 1 or 2 bytes wide, its
   * planes go from memory straight into an LDS ring several planes ahead of the arithmetic
   * (no staging registers, counted waits); 0: the register-staged form everywhere.  Same
   * arithmetic function, same results bit for bit. */
  IFE_OPT_FEAT_RING = 10,
  /* Upper bound in MiB on the scratch of the dense bag calls (the planes of the box passes and,
   * in ife_bag_image_dense, the features of a group of scales): 0 (default) sizes the groups
   * from the free device memory.  Bins and scales then go through in smaller groups; results
   * never change.  The dense bag stream takes its budget from it too (read by _begin): features,
   * codes, and of the rest an eighth as the default bound of a block. */
  IFE_OPT_DENSE_SCRATCH_MB = 11,
  /* 1 (default): the first axis pass (Z) of ife_emphysema_features and of its streaming form
   * runs ONE causal sweep per line for all scales of a group, straight from image and mask (no
   * cast / multiply prepass; that launch also leaves the two float sources), and the line
   * kernel proper then makes backward sweeps only.  In force with IFE_OPT_IIR_CKPT 2.  0: the
   * prepass, and every (scale, field) job sweeps forward on its own.  Same results bit for
   * bit. */
  IFE_OPT_Z_SWEEP = 12,
  /* 0 (default) or 1 (anything else: IFE_E_ARG): the feature path the COMPOSITE calls run
   * internally.  With 1, ife_samples_add_image, ife_bag_image, ife_bag_image_dense,
   * ife_bag_dense_stream_begin (and so _next) and ife_emphysema_features_begin / _fetch / _end
   * give bit for bit what their documented composition gives when ife_differential_features
   * stands in for ife_emphysema_features: the same mask handed over (labels clamped to {0,1} in
   * the bag and sample calls, the caller's mask in the scale stream), the context's trig mode,
   * the same component order and masking rule (mask != 0 ? v : 0).  The sample columns and the
   * dense bin codes are then written straight from the jet (csrc/feature_kernels.hpp:
   * jet_samples_kernel, jet_codes_kernel_*): no feature volume exists in the all-foreground
   * sample branch or in the dense calls, whose budget has no feature share (the jet workspace,
   * 140 bytes per voxel, lies outside IFE_OPT_DENSE_SCRATCH_MB as the finite-difference
   * workspace does).  A stream takes the value in force at its _begin; setting the option
   * between _begin and _fetch / _next changes nothing of what that stream delivers.
   * ife_emphysema_features, ife_differential_features, the jet and every ife_stage_* call name
   * their arithmetic and ignore the option.  The composite calls run the differential path on one
   * device: ife_multi_set_option refuses the value 1 (ife_multi_differential_features names its
   * arithmetic and runs on several).  With 0 every call does exactly what it did
   * before the option existed.  The library reads no environment variable for it (the host
   * Engine maps IFE_DIFFERENTIAL onto it). */
  IFE_OPT_DIFFERENTIAL = 13
} ife_option;

typedef struct {
  int64_t nx, ny, nz; /* size in voxels */
  double sx, sy, sz;  /* spacing (physical units per voxel), > 0 */
} ife_volume_desc;

/* number of feature components, ImageToEmphysemaFeaturesFilter.h:62 (numFeatures) */
#define IFE_NUM_FEATURES 8
/* component order of ife_emphysema_features, ExtractFeatures.cxx:126-130 */
#define IFE_FEATURE_NAMES                                                              \
  {"GaussianBlur", "GradientMagnitude", "Eigenvalue1", "Eigenvalue2", "Eigenvalue3",   \
   "LaplacianOfGaussian", "GaussianCurvature", "FrobeniusNorm"}

/* ---- context ----------------------------------------------------------------- */

int ife_abi_version(void);
/* Creates a context on HIP device `device`.  Replaces nothing in the reference
 * (which has no device); it owns the workspace the ITK mini-pipeline would hold as
 * intermediate images (ImageToEmphysemaFeaturesFilter.h:74-117). */
int ife_ctx_create(int device, ife_ctx **ctx);
void ife_ctx_destroy(ife_ctx *ctx);
/* Last error text of this context (or of ife_ctx_create when ctx is NULL).
 * Stands in for itk::ExceptionObject::what() (ExtractFeatures.cxx:145-152). */
const char *ife_last_error(const ife_ctx *ctx);
/* Borrow a hipStream_t for all later launches (NULL = the default stream). */
int ife_ctx_set_stream(ife_ctx *ctx, void *hip_stream);
int ife_ctx_set_option(ife_ctx *ctx, int option, int value);
/* Grow the workspace for volumes of this size now (so that later DEVICE-mode calls
 * allocate nothing). */
int ife_ctx_reserve(ife_ctx *ctx, const ife_volume_desc *vol);
/* Block until everything enqueued by this context has finished. */
int ife_ctx_synchronize(ife_ctx *ctx);

/* ---- a1 / a2: per-voxel numerics ----------------------------------------------- */

/* Symmetric3x3EigenvalueSolver<float>::operator()
 * (include/ife/Numerics/Symmetric3x3EigenvalueSolver.h:33-132) on n matrices.
 * A6: n x (xx,xy,xz,yy,yz,zz); ev3: n x 3, |ev0| >= |ev1| >= |ev2|. */
int ife_eigenvalues(ife_ctx *ctx, const float *A6, int64_t n, float *ev3, int mem);
/* EigenvalueFeaturesFunctor<float>::operator()
 * (include/ife/Numerics/EigenvalueFeaturesFunctor.h:20-31): f6 = n x
 * (ev0, ev1, ev2, sum, product, sqrt(sum of squares)). */
int ife_eigenvalue_features(ife_ctx *ctx, const float *A6, int64_t n, float *f6, int mem);

/* ---- a3: Hessian3DImageFilter --------------------------------------------------- */

/* itk::Hessian3DImageFilter<Image<float,3>,VectorImage<float,3>>: SetInput + Update
 * + GetOutput (include/ife/Filters/Hessian3DImageFilter.h:23-28,
 * Hessian3DImageFilter.hxx:13-60,80-97).  out6: 6 comps xx,xy,xz,yy,yz,zz. */
int ife_hessian3d(ife_ctx *ctx, const float *image, const ife_volume_desc *vol, float *out6,
                  int layout, int mem);

/* itk::GradientMagnitudeImageFilter as wired at
 * ImageToEmphysemaFeaturesFilter.hxx:27-28 / FiniteDifference_GradientFeatures.cxx:104-106 */
int ife_gradient_magnitude(ife_ctx *ctx, const float *image, const ife_volume_desc *vol,
                           float *out, int mem);

/* ---- a4: NormalizedGaussianConvolutionImageFilter ------------------------------- */

/* SetInputImage + SetInputCertainty + SetSigma + Update
 * (include/ife/Filters/NormalizedGaussianConvolutionImageFilter.h:86-93,
 * NormalizedGaussianConvolutionImageFilter.hxx:40-63):
 * out = G_sigma(image*certainty) / G_sigma(certainty), G = ITK recursive Gaussian
 * run Z, X, Y; zero denominator -> FLT_MAX.  Every axis must be >= 4 voxels.
 * sigma is double here (ScalarRealType of the Gaussian filter, .h:75,92-93; the
 * MaskedNormalizedConvolution tool parses doubles, :117) and float in
 * ife_emphysema_features (ScalarRealType = PixelType there, .h:41,58-59). */
int ife_normalized_gaussian_convolution(ife_ctx *ctx, const float *image,
                                        const float *certainty, const ife_volume_desc *vol,
                                        double sigma, float *out, int mem);

/* ---- f4: differential normalized convolution ---------------------------------------- */

/* The derivative form the reference sketches but does not implement
 * (include/ife/Filters/NormalizedGaussianConvolutionImageFilter.h:28-44):
 *   out = ({a_x*cT}{a*c} - {a_x*c}{a*cT}) / {a*c}^2  / spacing[axis]
 * a = the recursive Gaussian of ife_normalized_gaussian_convolution (axes z, x, y), a_x = the
 * same with ITK's FirstOrder recursive Gaussian along `axis` (0 = x, 1 = y, 2 = z; pixel units,
 * hence the division by the spacing).  Float arithmetic as written; {a*c}^2 == 0 -> FLT_MAX. */
int ife_differential_normalized_convolution(ife_ctx *ctx, const float *image,
                                            const float *certainty, const ife_volume_desc *vol,
                                            double sigma, int axis, float *out, int mem);

/* The complete form of that sketch: U = {a*cT}/{a*c} with its gradient and Hessian by the quotient
 * rule, differentiating the applicability and never the result (no value of U outside the
 * certainty's support enters a derivative).  cT = image * certainty (float).  For f in {cT, c} and
 * every order triple (ox, oy, oz) with ox + oy + oz <= 2:
 *   F[ox,oy,oz](f) = RG_y^oy(RG_x^ox(RG_z^oz(f)))
 * RG_axis^order = ITK's recursive Gaussian of that order along that axis (pixel units), passes in
 * the order z, x, y, a float image between passes, sigma in physical units.  N = F(cT), D = F(c),
 * r_i = 1.0 / spacing_i.  Per voxel in double, every operation rounded on its own, in this order:
 *   d    = D[000]
 *   U    = N[000] / d
 *   U_i  = (N[e_i] - U * D[e_i]) / d                                            i = x, y, z
 *   U_ij = (((N[e_i+e_j] - U_i * D[e_j]) - U_j * D[e_i]) - U * D[e_i+e_j]) / d   i <= j
 *   g_i  = U_i * r_i
 *   h_ij = U_ij * (r_i * r_j)
 * out10: the ten components (float)U, g_x, g_y, g_z, h_xx, h_xy, h_xz, h_yy, h_yz, h_zz in
 * `layout`; all ten are FLT_MAX where the stored float D[000] == 0 (the Div functor's rule, as in
 * the two calls above).  Every axis must be >= 4 voxels.  IFE_MEM_DEVICE: the interleaved output
 * must be aligned to 8 bytes.  Workspace: 140 bytes per voxel (csrc/diff_capi.inc); IFE_E_NOMEM
 * when it does not fit. */
int ife_normalized_convolution_jet(ife_ctx *ctx, const float *image, const float *certainty,
                                   const ife_volume_desc *vol, double sigma, float *out10, int layout,
                                   int mem);

/* ---- a5 + a9: ImageToEmphysemaFeaturesFilter, one execution per scale ------------ */

/* SetInputImage + SetInputMask + for each sigma {SetSigma; Update; GetOutput}
 * (include/ife/Filters/ImageToEmphysemaFeaturesFilter.h:44-62,
 * ImageToEmphysemaFeaturesFilter.hxx:15-55,99-121; scale loop
 * tools/ExtractFeatures.cxx:132-154).
 * image: IFE_F32 or IFE_I16 (converted exactly to float on load);
 * mask: IFE_U8 or IFE_U16, value used as certainty weight and tested != 0 for the
 * final masking; NULL means all ones.
 * out: n_sigmas consecutive 8-component volumes (scale-major), each in `layout`. */
int ife_emphysema_features(ife_ctx *ctx, const void *image, int image_dtype, const void *mask,
                           int mask_dtype, const ife_volume_desc *vol, const float *sigmas,
                           int n_sigmas, float *out, int layout, int mem);

/* The same eight features (order of IFE_FEATURE_NAMES) from the jet of
 * ife_normalized_convolution_jet instead of finite differences of the smoothed value, which next
 * to the mask border read the normalized convolution where it is an extrapolation.  No
 * counterpart in the reference.  Per voxel: S = (float)U; G = (float)sqrt((g_x*g_x + g_y*g_y) +
 * g_z*g_z) in double; the six float h through EigenvalueFeaturesFunctor<float> in the context's
 * trig mode; every component mask != 0 ? v : 0.  Arguments, certainty (the mask value, NULL = all
 * ones), output order and alignment as in ife_emphysema_features.  A voxel with mask != 0 and
 * D[000] == 0 gets the features of a jet of ten FLT_MAX.  Scales run one after the other. */
int ife_differential_features(ife_ctx *ctx, const void *image, int image_dtype, const void *mask,
                              int mask_dtype, const ife_volume_desc *vol, const float *sigmas,
                              int n_sigmas, float *out, int layout, int mem);

/* The scale loop of tools/ExtractFeatures.cxx:132-154 as a stream: _begin uploads image and
 * mask ONCE (host pointers), runs Cast + Multiply once and enqueues every scale, leaving the
 * outputs in device memory owned by the context; _fetch(scale) blocks until that scale has
 * finished and copies its 8-component volume (`layout` of _begin) to host memory on a copy
 * stream of its own -- so a caller can write scale k to disk while the device is still busy
 * with the later scales, and never holds more than one scale in host memory; _end frees the
 * device copy (also done by the next _begin and by ife_ctx_destroy).  IFE_E_STATE when a
 * scale is fetched that _begin did not start.  _begin returns once image and mask have been
 * copied to the device (the scales are still running): the caller may overwrite or free them
 * from then on, page-locked memory included; `out` must stay valid until its _fetch returns.
 * With IFE_OPT_DIFFERENTIAL at 1 when _begin is called, every scale is that of
 * ife_differential_features (the value at _begin decides for the whole stream). */
int ife_emphysema_features_begin(ife_ctx *ctx, const void *image, int image_dtype,
                                 const void *mask, int mask_dtype, const ife_volume_desc *vol,
                                 const float *sigmas, int n_sigmas, int layout);
int ife_emphysema_features_fetch(ife_ctx *ctx, int scale, float *out);
int ife_emphysema_features_end(ife_ctx *ctx);

/* ---- DEFLATE blocks formed on the device (row f3: the volume writer's compression) ----
 *
 * ife_deflate turns `bytes` bytes into complete, non-final DEFLATE blocks (RFC 1951) that start
 * and end on a byte boundary: with 03 00 appended they are a raw DEFLATE stream that any inflater
 * accepts, and a gzip member once a header in front and CRC-32 and length behind are added.  The
 * output depends on the input bytes alone.
 *
 * The format.  The input is cut into chunks of 32768 bytes (the last may be shorter); the blocks
 * of the chunks are concatenated in order.  Tokens of a chunk [lo, hi): eq[i] holds when i >= 4
 * and b[i] == b[i-4] (i counts from the start of the input, so a match may reach back over the
 * chunk start).  Where eq is false the byte is a literal.  A maximal run [i, j) of true eq with
 * j <= hi (a run running at lo starts at lo) of length L >= 3 becomes matches of distance 4 and
 * length min(258, rest) while rest >= 3, and the 0, 1 or 2 bytes left over are literals; a run
 * shorter than 3 is literals.  Form F: one block with the fixed Huffman codes (BFINAL 0, BTYPE
 * 01), the tokens, end of block, then an empty stored block to realign (three zero bits, zero
 * padding to the byte boundary, 00 00 FF FF).  Form S: one stored block, 00, LEN, NLEN, the
 * chunk's bytes: 5 + len bytes.  A chunk takes S when S is not longer than F, so the output is at
 * most ife_deflate_bound(bytes) = bytes + 5 * ceil(bytes / 32768) bytes; no input gives no output.
 *
 * `data` and `out` follow `mem` and may have any byte alignment, on the device too; `out_bytes`
 * and `crc32` are host scalars, *crc32 the CRC-32 (IEEE, as zlib's crc32) of the input.  The call
 * blocks.  A `capacity` below the size of the blocks returns IFE_E_SIZE with the needed size in
 * *out_bytes and nothing written to `out`. */
size_t ife_deflate_bound(size_t bytes);
int ife_deflate(ife_ctx *ctx, const void *data, size_t bytes, void *out, size_t capacity,
                size_t *out_bytes, uint32_t *crc32, int mem);

/* One component plane (0 .. 7) of a scale of the stream as the blocks of ife_deflate, to host
 * memory: between ife_emphysema_features_begin with IFE_PLANAR (IFE_E_STATE for an interleaved
 * stream, whose components are not contiguous) and _end.  It waits for that scale on the stream's
 * copy stream, forms the blocks there and copies only them, so later scales keep computing.
 * `capacity`, `out_bytes` and `crc32` as in ife_deflate. */
int ife_emphysema_features_fetch_deflated(ife_ctx *ctx, int scale, int component, void *out,
                                          size_t capacity, size_t *out_bytes, uint32_t *crc32);

/* ---- a6 / a7 / a8: tool bodies ---------------------------------------------------- */

/* Body of tools/FiniteDifference_HessianFeatures.cxx:126-229 (un-smoothed Hessian,
 * eigen features, mask==0 -> six zeros), with Hessian3DImageFilter.hxx:34-37 as the
 * normative derivative wiring (the tool's :155 direction slip is not reproduced).
 * out6 comps: eig1, eig2, eig3, LoG, Curvature, Frobenius.  mask may be NULL. */
int ife_fd_hessian_features(ife_ctx *ctx, const void *image, int image_dtype,
                            const void *mask, int mask_dtype, const ife_volume_desc *vol,
                            float *out6, int layout, int mem);
/* Body of tools/FiniteDifference_GradientFeatures.cxx:104-113: the mask is a float
 * image there. */
int ife_fd_gradient_features(ife_ctx *ctx, const float *image, const float *mask,
                             const ife_volume_desc *vol, float *out, int mem);
/* Body of tools/MaskedImageFilter.cxx:75-93 (double pixels, -v outside value). */
int ife_mask_image_f64(ife_ctx *ctx, const double *image, const double *mask, double outside,
                       int64_t n, double *out, int mem);

/* ---- stage entry points: Z-slab decomposition across GPUs ----------------------------
 *
 * The reference runs the path in one address space (it has no
 * distributed code).  A multi-GPU host cuts the volume into Z-slabs, one per device, and
 * interposes two neighbour exchanges between these stages (image-feature-extraction_amd/
 * slab.py, csrc/multi_capi.inc, DESIGN.md "Multi-GPU"): the state of the Z recursion (the only
 * one that crosses slabs) handed from slab to slab, 32 bytes per line and job, and a
 * one-plane halo exchange in front of the stencil.  All pointers are device memory; calls
 * enqueue on the context's stream and do not synchronise. */

/* CastImageFilter + MultiplyImageFilter (ImageToEmphysemaFeaturesFilter.hxx:21,110;
 * NormalizedGaussianConvolutionImageFilter.hxx:48-49) on a slab: tc = float(image) *
 * float(mask), cf = float(mask).  mask NULL: tc = float(image), cf untouched (may be NULL).
 * y_chunks = 1: outputs in the slab's own order.  y_chunks = W > 1: outputs in the order an
 * all-to-all sends from, [W][nz][ny/W][nx] (chunk h = the rows of rank h's Y-slab), so the
 * host needs no packing pass. */
int ife_stage_prepare(ife_ctx *ctx, const void *image, int image_dtype, const void *mask,
                      int mask_dtype, const ife_volume_desc *slab, int y_chunks, float *tc,
                      float *cf);
/* One axis of itk::SmoothingRecursiveGaussianImageFilter (the reference reaches it at
 * NormalizedGaussianConvolutionImageFilter.hxx:51-55); axis 0 = x, 1 = y, 2 = z; the
 * caller keeps ITK's order z, x, y.  Not in place. */
int ife_stage_recursive_gaussian(ife_ctx *ctx, const float *in, float *out,
                                 const ife_volume_desc *vol, int axis, double sigma);
/* One axis pass of itk::RecursiveGaussianImageFilter of order 0 (ZeroOrder, the call above), 1
 * (FirstOrder) or 2 (SecondOrder), NormalizeAcrossScale off: the derivative filters answer in
 * pixel units along `axis`.  IFE_E_ARG for any other order.  Not in place. */
int ife_stage_recursive_gaussian_order(ife_ctx *ctx, const float *in, float *out,
                                       const ife_volume_desc *vol, int axis, double sigma, int order);
/* The same over njobs (<= 8) float volumes of one geometry in a single launch, each with
 * its own sigma: numerator and denominator of several scales.  A slab host needs this to
 * keep the device full (a 64-plane slab has too few lines for one job per launch).
 * in_y_chunks = W > 1 (axis 0 only): every input is the Y-chunked image of the slab as the
 * all-to-all back from the Z pass leaves it, [W][nz][ny/W][nx]; the outputs are plain
 * slabs.  Needs (ny/W) % 64 == 0.  in_y_chunks = 1: plain inputs. */
int ife_stage_recursive_gaussian_batch(ife_ctx *ctx, int njobs, const float *const *in,
                                       float *const *out, const ife_volume_desc *vol, int axis,
                                       const double *sigmas, int in_y_chunks);
/* The Z pass of a Z-slab with the recursion state handed across the slab boundaries (the
 * reference has no counterpart: its RecursiveGaussianImageFilter sees whole lines,
 * NormalizedGaussianConvolutionImageFilter.hxx:51-55).  A slab holds planes [z0, z1) of every
 * Z line; `in` are njobs (<= 8) float slabs [nz][ny][nx] with one sigma each.  Three calls
 * (or two: ife_stage_z_fused below replaces the later sweep and the combine):
 *   ife_stage_z_sweep(direction 0): causal recursion upwards.  has_neighbour = a slab below
 *     exists and state_in holds its outgoing record; else ITK's start-of-line rule applies.
 *     Leaves the causal checkpoints in ck[job] and the state at z1 in state_out.
 *   ife_stage_z_sweep(direction 1): anticausal recursion downwards, state_in from the slab
 *     above (or ITK's end-of-line rule); anticausal checkpoints, state at z0 in state_out.
 *   ife_stage_z_combine: rebuilds both recursions of every block pair from the checkpoints
 *     and writes float(causal + anticausal) to out[job].
 * Stitched over the slabs this is bit for bit the sequential recursion of the whole line.
 * Lines [line0, line0 + nlines) of the nx*ny lines are processed (x-fastest line index), so
 * that a host can pipeline groups of lines across devices.  A state buffer holds, per job,
 * 4*nlines doubles y[k][line] (IFE_Z_STATE_BYTES * nlines bytes; 8-byte aligned): the last
 * four outputs of the recursion, nearest first.  The INPUT samples a state refers to do not
 * travel with it: where a neighbour exists, `in[job]` must be preceded by the neighbour's last
 * 3 planes (has_lo / direction 0) and followed by its first 4 planes (has_hi / direction 1) --
 * the slab's input is cut from the volume with that overlap (IFE_Z_OVERLAP_LO / _HI planes),
 * which every device can do from its own copy of the raw data, and `in[job]` points at the
 * slab's own plane 0 inside it.  ck[job] points at ife_stage_z_ck_bytes(slab) bytes of device
 * memory that must survive from the sweeps to the combine.  Every slab needs at least 4
 * planes. */
#define IFE_Z_STATE_BYTES 32
#define IFE_Z_OVERLAP_LO 3
#define IFE_Z_OVERLAP_HI 4
size_t ife_stage_z_ck_bytes(const ife_volume_desc *slab);
int ife_stage_z_sweep(ife_ctx *ctx, int direction, int njobs, const float *const *in,
                      const ife_volume_desc *slab, int64_t line0, int64_t nlines,
                      const double *sigmas, int has_neighbour, const void *state_in,
                      void *state_out, void *const *ck);
int ife_stage_z_combine(ife_ctx *ctx, int njobs, const float *const *in, float *const *out,
                        const ife_volume_desc *slab, int64_t line0, int64_t nlines,
                        const double *sigmas, int has_lo, int has_hi, void *const *ck);
/* Sweep of `direction` and combine in one: for the direction whose state reaches a slab LAST.
 * The recursion of `direction` runs through the slab from state_in (or ITK's border rule where
 * that side has no neighbour: has_lo for direction 0, has_hi for direction 1), the other
 * direction's values come from the checkpoints its ife_stage_z_sweep left in ck[job]; writes
 * float(causal + anticausal) to out[job] and the carried state to state_out.  Three recursion
 * steps per sample for the slab (one lean sweep + this) instead of four (two sweeps + combine),
 * the same operations on every sample: same bits. */
int ife_stage_z_fused(ife_ctx *ctx, int direction, int njobs, const float *const *in,
                      float *const *out, const ife_volume_desc *slab, int64_t line0, int64_t nlines,
                      const double *sigmas, int has_lo, int has_hi, const void *state_in,
                      void *state_out, void *const *ck);
/* The three calls above with an order per job: orders[job] is 0 (ZeroOrder), 1 (FirstOrder) or 2
 * (SecondOrder) as in ife_stage_recursive_gaussian_order; NULL means all zero, which is exactly
 * the call above; any other value is IFE_E_ARG.  The recurrence has the same form for every
 * order (four input taps, four feedback taps; only the coefficients differ), so state records,
 * overlap planes and checkpoints are those of order 0, and the contract is the same: stitched
 * over the slabs the result is bit for bit ife_stage_recursive_gaussian_order along z on the
 * whole volume, for every order.
 * ife_stage_z_sweep_order reads each plane ONCE for three consecutive jobs that have the same
 * `in`, the same sigma and the orders 0, 1, 2 in that order (the three Z-level fields the
 * differential path takes of one source): one lane then advances the three recursions side by
 * side.  Every other job runs as in ife_stage_z_sweep.  Checkpoints, states and therefore every
 * later result are the same bit for bit in either form; the job order only decides the form. */
int ife_stage_z_sweep_order(ife_ctx *ctx, int direction, int njobs, const float *const *in,
                            const ife_volume_desc *slab, int64_t line0, int64_t nlines,
                            const double *sigmas, const int *orders, int has_neighbour,
                            const void *state_in, void *state_out, void *const *ck);
int ife_stage_z_combine_order(ife_ctx *ctx, int njobs, const float *const *in, float *const *out,
                              const ife_volume_desc *slab, int64_t line0, int64_t nlines,
                              const double *sigmas, const int *orders, int has_lo, int has_hi,
                              void *const *ck);
int ife_stage_z_fused_order(ife_ctx *ctx, int direction, int njobs, const float *const *in,
                            float *const *out, const ife_volume_desc *slab, int64_t line0, int64_t nlines,
                            const double *sigmas, const int *orders, int has_lo, int has_hi,
                            const void *state_in, void *state_out, void *const *ck);
/* The last axis pass of the normalized convolution in its quotient form
 * (NormalizedGaussianConvolutionImageFilter.hxx:51-61: the two smoothings and the Div functor):
 * job j filters num[j] and den[j] along `axis` (1 = y or 2 = z) with sigmas[j] and stores
 * numerator / denominator (denominator == 0: the functor's max()) in out[j].  njobs <= 4. */
int ife_stage_recursive_gaussian_quotient(ife_ctx *ctx, int njobs, const float *const *num,
                                          const float *const *den, float *const *out,
                                          const ife_volume_desc *vol, int axis, const double *sigmas);

/* Everything after the smoothing (ImageToEmphysemaFeaturesFilter.hxx:27-54 plus the
 * Divide of NormalizedGaussianConvolutionImageFilter.hxx:57-61) on a slab of slab->nz
 * planes.  num/den hold halo_lo + slab->nz + halo_hi planes: with halo_lo (halo_hi) = 1
 * the first (last) plane is the neighbouring slab's boundary plane, with 0 the boundary
 * is replicated as at the end of the volume.  den NULL: certainty == 1.  mask/out cover
 * the slab's own planes only. */
int ife_stage_features(ife_ctx *ctx, const float *num, const float *den, const void *mask,
                       int mask_dtype, const ife_volume_desc *slab, int halo_lo, int halo_hi,
                       float *out, int layout);

/* Everything of ife_differential_features behind the Z level, on a slab: zf[3*s + k] is the
 * Z-level field of source s (0 = cT = float(image) * float(mask), 1 = c = float(mask), or the
 * constant 1.0f without a mask) at order k, on the slab's own planes (what the ife_stage_z_*_order
 * calls leave).  Runs the X level (12 fields), the Y level (20 fields) and the pointwise feature
 * kernel in the context's trig mode: the code path and slot schedule of the one-device call behind
 * its Z launch, so on one slab that is the whole volume the result is that call's bit for bit, and
 * over several slabs too, since nothing behind the Z level crosses a plane.  Workspace: that of
 * ife_differential_features on a volume of the slab's size, less its Z-level fields and sources.
 * mask (NULL: all ones) and out cover the slab's planes; pointer alignment as in
 * ife_differential_features (mask to its element size, interleaved out to 16 bytes); nx, ny >= 4. */
int ife_stage_jet_features(ife_ctx *ctx, const float *const zf[6], const void *mask, int mask_dtype,
                           const ife_volume_desc *slab, double sigma, float *out, int layout);

/* ---- several devices in one process --------------------------------------------------
 *
 * The same Z-slab decomposition driven from C++ by ONE host thread: device r of the list
 * owns the r-th range of planes (nz / n planes each, remainder on the first ones; every
 * slab needs 4), states and stencil planes travel by peer copies over xGMI, every dependency
 * is a HIP event.  Host pointers in, host pointers out; blocks until the whole output is
 * there.  Same results bit for bit as ife_emphysema_features on one device.  A device may be
 * listed more than once (how a one-GPU box tests n > 1). */
typedef struct ife_multi ife_multi;
int ife_multi_create(const int *devices, int n_devices, ife_multi **out);
void ife_multi_destroy(ife_multi *m);
const char *ife_multi_last_error(const ife_multi *m);
/* ife_ctx_set_option on every context of the engine.  IFE_OPT_DIFFERENTIAL 1 is IFE_E_ARG: the
 * option selects the path of the COMPOSITE calls, and those run the differential path on one device
 * (0 is accepted).  The call that names its arithmetic exists here as it does on one device:
 * ife_multi_differential_features below. */
int ife_multi_set_option(ife_multi *m, int option, int value);
int ife_multi_emphysema_features(ife_multi *m, const void *image, int image_dtype,
                                 const void *mask, int mask_dtype, const ife_volume_desc *vol,
                                 const float *sigmas, int n_sigmas, float *out, int layout);
/* The scale loop of tools/ExtractFeatures.cxx:132-154 over several devices, one scale at a
 * time to the host (the multi-device form of ife_emphysema_features_begin / _fetch / _end):
 * _begin uploads every slab once, runs Cast + Multiply once and enqueues every scale on every
 * device without waiting; _fetch(k) blocks until scale k of every slab has been copied into
 * `out` (that scale's whole volume: nx*ny*nz*8 floats of host memory) on a stream of its own,
 * while the later scales keep computing; _end drains.  IFE_E_STATE out of sequence.  As with
 * ife_emphysema_features_begin, image and mask may be reused as soon as _begin returns. */
int ife_multi_emphysema_features_begin(ife_multi *m, const void *image, int image_dtype,
                                       const void *mask, int mask_dtype, const ife_volume_desc *vol,
                                       const float *sigmas, int n_sigmas, int layout);
int ife_multi_emphysema_features_fetch(ife_multi *m, int scale, float *out);
int ife_multi_emphysema_features_end(ife_multi *m);
/* ife_differential_features over the devices of the engine: same arguments, checks and errors as
 * ife_multi_emphysema_features (every slab needs 4 planes: IFE_E_SIZE), host pointers in and out,
 * blocks; the result equals ife_differential_features on one device bit for bit.  Every slab is
 * uploaded with its overlap planes and cT and c are built over them; a scale is six Z jobs (cT and
 * c at orders 0, 1, 2), carried through the two state chains like the two jobs of the
 * finite-difference path; behind them every rank runs ife_stage_jet_features on its own planes.
 * No plane is exchanged.  _begin is the streaming form; it shares
 * ife_multi_emphysema_features_fetch / _end and their IFE_E_STATE rules. */
int ife_multi_differential_features(ife_multi *m, const void *image, int image_dtype,
                                    const void *mask, int mask_dtype, const ife_volume_desc *vol,
                                    const float *sigmas, int n_sigmas, float *out, int layout);
int ife_multi_differential_features_begin(ife_multi *m, const void *image, int image_dtype,
                                          const void *mask, int mask_dtype, const ife_volume_desc *vol,
                                          const float *sigmas, int n_sigmas, int layout);

/* ---- rows f1 / f2: sample columns, equalizing histogram edges, dense histograms ------- *
 * The immediate consumer of the feature volume.  The samples never
 * leave HBM; only the nbins-1 edges per column come back.                                 */

/* std::sort of one sample column
 * (tools/DetermineHistogramBinEdges_MultiScaleEigenvalueFeatures.cxx:284).  Ascending;
 * -0 sorts before +0 (std::sort leaves their order unspecified).  in == out is allowed. */
int ife_sort_f32(ife_ctx *ctx, const float *in, int64_t n, float *out, int mem);

/* determineEdgesForEqualizedHistogram(first, last, d_first, nBins),
 * include/ife/Statistics/DetermineEdgesForEqualizedHistogram.h:21-137.  sorted[0..n) must
 * be ascending; writes nbins-1 edges.  IFE_E_ARG when n < nbins (std::out_of_range there,
 * :36-38); IFE_E_STATE when the walk would pass the last sample (an assert there, :74). */
int ife_equalized_edges_f32(ife_ctx *ctx, const float *sorted, int64_t n, int nbins,
                            float *edges, int mem);
/* the same on doubles (the reference's own test instantiates the template on double,
 * test/DetermineEdgesForEqualizedHistogramTest.cxx:11) */
int ife_equalized_edges_f64(ife_ctx *ctx, const double *sorted, int64_t n, int nbins,
                            double *edges, int mem);

/* DenseHistogram<float>: insert every value, getCounts
 * (include/ife/Statistics/DenseHistogram.h:29-64).  Bins (-inf,e0], (e0,e1], ...,
 * (e_last,inf); counts holds n_edges+1 entries; 1 <= n_edges <= 1024. */
int ife_dense_histogram_f32(ife_ctx *ctx, const float *edges, int n_edges, const float *values,
                            int64_t n, uint32_t *counts, int mem);

/* Row f2: the bag rows of tools/MakeBag.cxx:405-472 for ONE feature volume.  rois holds
 * n_rois boxes {x, y, z, sx, sy, sz} (index and size in voxels, as ROIReader.hxx:28-47 reads
 * them); for every box and component c the component values of the box's voxels with
 * mask != 0 are binned by edges[c*n_edges ..] (DenseHistogram bins), into
 * counts[(roi*ncomp + c)*(n_edges+1) + bin].  IFE_E_ARG when a box leaves the volume
 * (RegionOfInterestImageFilter throws there).  ncomp*(2*n_edges+1) <= 8192. */
int ife_roi_histograms(ife_ctx *ctx, const float *features, int layout, int ncomp,
                       const void *mask, int mask_dtype, const ife_volume_desc *vol,
                       const int64_t *rois, int n_rois, const float *edges, int n_edges,
                       uint32_t *counts, int mem);
/* One image of MakeBag: labels clamped to {0,1} (:236-244), a5 at every scale with the
 * features left in HBM, then the rows above per scale.  rois, edges ([n_sigmas*8][n_edges],
 * the rows of the histogram specification) and counts
 * ([n_rois][n_sigmas*8][n_edges+1]) are HOST arrays; mem describes image and mask.
 * IFE_OPT_DIFFERENTIAL 1: ife_differential_features in place of a5. */
int ife_bag_image(ife_ctx *ctx, const void *image, int image_dtype, const void *mask,
                  int mask_dtype, const ife_volume_desc *vol, const float *sigmas, int n_sigmas,
                  const int64_t *rois, int n_rois, const float *edges, int n_edges,
                  uint32_t *counts, int mem);

/* ---- the dense bag: one region per mask voxel (tools/MakeBagDense.cxx:239-250) ------------- *
 * Conventions of the three calls: size = {sx, sy, sz} in voxels, each >= 1.  Voxel (x, y, z) is a
 * centre when gen_mask != 0 there and the box [x - sx/2, x - sx/2 + sx) x [y - sy/2, ...) x
 * [z - sz/2, ...) lies inside the volume; the division is integer division
 * (include/ife/ROI/DenseROIGenerator.hxx:35-40), so even sizes are off-centre by design.  Regions
 * are numbered in raster order of their centres, x fastest.  A box larger than the volume gives
 * zero regions, which is not an error.  Masks are IFE_U8 or IFE_U16.  Volumes of up to 2^32-1
 * voxels (regions are numbered in 32 bits; IFE_E_SIZE beyond); the number of regions is not
 * limited to int.  The calls block in both memory modes (the region count comes to the host). */

/* DenseROIGenerator<TMask>::generate(size): the boxes {x0,y0,z0,sx,sy,sz} of all centres.
 * rois == NULL: only *n_rois is written.  Otherwise up to `capacity` boxes are written;
 * IFE_E_SIZE (with *n_rois set, nothing written) when there are more.  gen_mask and rois follow
 * `mem`, *n_rois is a HOST scalar. */
int ife_dense_rois(ife_ctx *ctx, const void *gen_mask, int gen_mask_dtype,
                   const ife_volume_desc *vol, const int64_t size[3],
                   int64_t *n_rois, int64_t *rois, int64_t capacity, int mem);

/* The rows ife_roi_histograms would give for those boxes, without the boxes:
 * counts[(roi*ncomp + c)*(n_edges+1) + bin], voxels with mask != 0 only, DenseHistogram bins (a
 * NaN value goes to bin 0, as there).  gen_mask NULL: mask decides the centres too.  Same capacity
 * rule (capacity in rows; IFE_E_SIZE with *n_rois set and nothing written); *n_rois is a HOST
 * scalar.  The counts are separable box sums of per-voxel bin codes (csrc/dense_kernels.hpp), so
 * the work per region does not depend on the box.
 * Limits: 1 <= n_edges <= 254 (IFE_E_ARG beyond): the bin of a voxel is kept in one byte and the
 * value 255 stands for "not in the mask".  The running sums are one byte wide after the x pass,
 * two after y and four after z: sx <= 255, sx*sy <= 65535 and sx*sy*sz <= 2^32-1 (IFE_E_SIZE
 * beyond; 41^3 and 101^3 are inside).  IFE_E_NOMEM when the scratch of one bin of one component
 * (4 bytes per voxel) does not fit. */
int ife_dense_roi_histograms(ife_ctx *ctx, const float *features, int layout, int ncomp,
                             const void *mask, int mask_dtype, const void *gen_mask,
                             int gen_mask_dtype, const ife_volume_desc *vol, const int64_t size[3],
                             const float *edges, int n_edges, uint32_t *counts,
                             int64_t capacity, int64_t *n_rois, int mem);

/* One image of MakeBagDense: ife_bag_image with the dense rule in place of the box list (labels
 * clamped to {0,1}, a5 at every scale, the rows above per scale).  edges and counts are HOST
 * arrays laid out as in ife_bag_image ([n_rois][n_sigmas*8][n_edges+1]); mem describes image,
 * mask and gen_mask.  Limits as for ife_dense_roi_histograms.  IFE_OPT_DIFFERENTIAL 1: the bin
 * codes of ife_differential_features, formed from the jet without a feature volume. */
int ife_bag_image_dense(ife_ctx *ctx, const void *image, int image_dtype, const void *mask,
                        int mask_dtype, const void *gen_mask, int gen_mask_dtype,
                        const ife_volume_desc *vol, const float *sigmas, int n_sigmas,
                        const int64_t size[3], const float *edges, int n_edges,
                        uint32_t *counts, int64_t capacity, int64_t *n_rois, int mem);

/* The same bag as a stream of row blocks, for bags that fit neither the device nor the host in one
 * piece.  Regions are numbered in raster order of their centres, so the regions whose centres lie
 * in a run of z planes are a contiguous range of rows; a block is such a run of whole planes (at
 * least one).  The device keeps the bin codes of all scales (one byte per voxel and column) and
 * counts one block at a time from them.
 *
 * _begin: arguments, limits and checks of ife_bag_image_dense (mem describes image, mask and
 * gen_mask; edges is a HOST array).  values: what _next delivers, the counts of
 * ife_bag_image_dense (uint32_t) or the frequencies of DenseHistogram::getFrequencies (float:
 * per histogram the counts summed into an int, then (float)count / (float)sum; an empty histogram
 * is NaN in every bin, sign and payload unspecified).  block_mb bounds the bytes of one block,
 * rows * n_sigmas*8 * (n_edges+1) * 4, in MiB (a single plane may exceed it); 0 takes the bound
 * from the scratch budget (IFE_OPT_DENSE_SCRATCH_MB, or the free device memory).  Writes the
 * number of regions to *n_rois and the row count of the largest block to *max_block_rows (both
 * HOST scalars), so that the caller can size one array.  Uploads the inputs, runs the features of
 * all scales and turns them into codes, plans the blocks and returns without waiting for any
 * counting; HOST inputs may be reused when it returns, DEVICE inputs once the first _next has
 * returned.  Zero regions (a box larger than the volume, too) is not an error: *n_rois = 0 and
 * the first _next reports the end.  A stream that is still open is dropped.
 *
 * _next: delivers the blocks in row order into the HOST array `rows`, laid out as in
 * ife_bag_image_dense: rows[(r - *row0) * n_sigmas*8 * (n_edges+1) + column * (n_edges+1) + bin]
 * for the rows r in [*row0, *row0 + *n_rows).  *n_rows = 0 says that the stream is finished, and
 * nothing else does.  capacity_rows smaller than the block: IFE_E_SIZE with *row0 and *n_rows
 * set and nothing consumed; the call may be repeated with a larger array.  While the block is
 * copied (on a copy stream of the stream's own) the next one is being counted.
 *
 * _end: frees what the stream holds on the device (also done by the next _begin and by
 * ife_ctx_destroy).  _next or _end without a _begin: IFE_E_STATE.
 *
 * The stream owns every buffer it uses between the calls, so any other call on the context is
 * legal between _begin and _end and does not change what the stream delivers.  Device memory:
 * the codes (nvox * n_sigmas*8 bytes), three block buffers (one planar that the counting fills,
 * two row-major on their way out) and the scratch of the box passes of one block.
 * IFE_OPT_DIFFERENTIAL 1 at _begin: the codes are those of ife_differential_features, formed from
 * the jet without a feature volume (the budget then has no feature share). */
typedef enum { IFE_BAG_COUNTS = 0, IFE_BAG_FREQUENCIES = 1 } ife_bag_values;
int ife_bag_dense_stream_begin(ife_ctx *ctx, const void *image, int image_dtype, const void *mask,
                               int mask_dtype, const void *gen_mask, int gen_mask_dtype,
                               const ife_volume_desc *vol, const float *sigmas, int n_sigmas,
                               const int64_t size[3], const float *edges, int n_edges,
                               int values, int block_mb, int64_t *n_rois,
                               int64_t *max_block_rows, int mem);
int ife_bag_dense_stream_next(ife_ctx *ctx, void *rows, int64_t capacity_rows, int64_t *row0,
                              int64_t *n_rows);
int ife_bag_dense_stream_end(ife_ctx *ctx);

/* ---- per-region label modes (tools/ExtractLabels.cxx:164-212) ------------------------------- *
 * The label of a region is the mode of a label volume (IFE_U8; anything else is IFE_E_ARG) inside
 * its box, given a set G of ignored labels (ignore[0..n_ignore), a HOST array, each in 0..255,
 * duplicates allowed, may be empty) and a dominant label d (`dominant`, < 0: none, > 255:
 * IFE_E_ARG).  n(l) is the number of voxels of the box that carry label l, l in 0..255; every
 * voxel counts, there is no counting mask.  c(l) = 0 if l is in G, else n(l).
 *   1. If d >= 0 and (n(d) > 0 or d is in G), the label is d.  (The reference asks
 *      counts.count(d) > 0 after it has inserted the ignored labels into its map, :189-198, so an
 *      ignored dominant label always wins.)
 *   2. Else, if max c > 0, the label is the smallest l with c(l) = max c.
 *   3. Else the label is the smallest member of G (every voxel of the box then carries an ignored
 *      label, and a box has at least one voxel, so G is not empty).
 * Where the maximum is unique this is what the reference computes.  Where it ties the reference
 * returns whichever key its std::unordered_map iterates first (:201-208), which depends on
 * insertion order and bucket count and not on the counts: parity is unpinned at ties, and "the
 * smallest label" is this library's definition.
 *
 * ife_roi_labels: rois holds n_rois boxes {x, y, z, sx, sy, sz} as in ife_roi_histograms,
 * out[n_rois] receives the labels; labels, rois and out follow `mem`.  IFE_E_ARG when a box leaves
 * the volume or has a size below 1, IFE_E_SIZE for a box of more than 2^32-1 voxels (in DEVICE mode
 * the boxes are checked on the device before they are used, and either fault is IFE_E_ARG); out is
 * not written then.  n_rois == 0 is IFE_OK with nothing written.  The call blocks in both memory
 * modes. */
int ife_roi_labels(ife_ctx *ctx, const void *labels, int labels_dtype, const ife_volume_desc *vol,
                   const int64_t *rois, int64_t n_rois, const int *ignore, int n_ignore,
                   int dominant, uint8_t *out, int mem);

/* out[r] = the label ife_roi_labels gives for the box ife_dense_rois numbers r, without the boxes:
 * the labels of a dense bag in the row order of the bag.  Centres, numbering, the zero-region
 * case, the capacity rule (capacity in labels; IFE_E_SIZE with *n_rois set and nothing written)
 * and the counter limits (sx <= 255, sx*sy <= 65535, sx*sy*sz <= 2^32-1) are those documented
 * above ife_dense_rois and ife_dense_roi_histograms.  out == NULL: only *n_rois is written.
 * gen_mask (IFE_U8 or IFE_U16) must not be NULL: there is no counting mask to fall back on.
 * labels, gen_mask and out follow `mem`; *n_rois is a HOST scalar.  All 256 label values are
 * served.  n(l) at every centre is a separable box sum (csrc/labels_kernels.hpp), so the work per
 * region does not depend on the box; beside the scratch of the box passes (sized from
 * IFE_OPT_DENSE_SCRATCH_MB or the free memory: 1 + 3 * labels-per-group bytes per voxel) the call
 * keeps 4 bytes per region.  IFE_E_NOMEM when the scratch of one label (4 bytes per voxel) does
 * not fit. */
int ife_dense_roi_labels(ife_ctx *ctx, const void *labels, int labels_dtype, const void *gen_mask,
                         int gen_mask_dtype, const ife_volume_desc *vol, const int64_t size[3],
                         const int *ignore, int n_ignore, int dominant, uint8_t *out,
                         int64_t capacity, int64_t *n_rois, int mem);

/* The tool's `samples( scales.size() * numFeatures )` (:165-166): one growing column per
 * (scale, feature), kept in device memory.  Belongs to the context it was created on. */
typedef struct ife_samples ife_samples;
int ife_samples_create(ife_ctx *ctx, int n_columns, ife_samples **out);
void ife_samples_destroy(ife_samples *s);
int ife_samples_count(const ife_samples *s, int column, int64_t *n);
int ife_samples_clear(ife_samples *s);

/* Append the ncomp feature values of the accepted voxels of one feature volume to columns
 * [first_column, first_column+ncomp).  indices == NULL: every voxel whose mask value
 * equals one of foreground[0..n_foreground) (the nSamples == 0 branch, :221-236;
 * 1 <= n_foreground <= 8).  indices != NULL: the listed voxels, x-fastest linear index,
 * repeats allowed (the sampled branch, :238-263: the host draws the positions).  Samples
 * are appended in raster order / list order, as the reference pushes them. */
int ife_samples_add_features(ife_ctx *ctx, ife_samples *s, int first_column,
                             const float *features, int layout, int ncomp, const void *mask,
                             int mask_dtype, int64_t nvox, const uint32_t *foreground,
                             int n_foreground, const int64_t *indices, int64_t n_indices,
                             int mem);

/* One image of the tool's loop (:176-265): the labels are clamped to {0,1} for the filter
 * (ClampImageFilter, :147-152), a5 runs at every scale, and the samples of scale i go to
 * columns [8i, 8i+8) -- in the all-foreground branch straight from the feature kernel (no
 * feature volume is stored), in the sampled branch from a feature volume left in HBM.  The samples object must have
 * 8*n_sigmas columns.  indices, when given, holds n_sigmas * n_indices_per_scale voxel
 * indices, scale-major.  IFE_OPT_DIFFERENTIAL 1: both branches take the features of
 * ife_differential_features (the all-foreground one straight from the jet, again without a
 * feature volume). */
int ife_samples_add_image(ife_ctx *ctx, ife_samples *s, const void *image, int image_dtype,
                          const void *mask, int mask_dtype, const ife_volume_desc *vol,
                          const float *sigmas, int n_sigmas, const uint32_t *foreground,
                          int n_foreground, const int64_t *indices,
                          int64_t n_indices_per_scale, int mem);

/* :282-289: sort every column and write its equalizing edges; edges is a HOST array of
 * n_columns * (nbins-1) floats, one row per column in column order. */
int ife_samples_sort(ife_ctx *ctx, ife_samples *s);
int ife_samples_equalized_edges(ife_ctx *ctx, ife_samples *s, int nbins, float *edges);
/* copy one column (count values) to a HOST array */
int ife_samples_read_column(ife_ctx *ctx, const ife_samples *s, int column, float *out,
                            int64_t capacity);

/* ---- signed distance map, expected distance ------------------------ */

/* itk::SignedMaurerDistanceMapImageFilter<Image<TMask,3>, Image<double,3>> as wired at
 * include/ife/Statistics/ExpectedDistanceFromCenterToInterestPoint.h:16-19 (BackgroundValue 0,
 * UseImageSpacing on).  mask: IFE_U8 or IFE_U16, foreground = mask != 0; NULL is IFE_E_ARG.
 * Sites are the foreground voxels with a background face neighbour inside the volume
 * (BinaryContourImageFilter, FullyConnected off); D2(v) = min over sites c of
 * ((hx(c)-hx(v))^2 + (hy(c)-hy(v))^2) + (hz(c)-hz(v))^2 with h(i) = (double)i * spacing, every
 * operation rounded on its own; out = +-(squared ? D2 : sqrt(D2)), positive where
 * (mask != 0) == (inside_is_positive != 0).  A volume without a site (all foreground or all
 * background) gives D2 = DBL_MAX everywhere, as ITK leaves it; that is not an error.  Any axis
 * length >= 1; nx <= 32768 (IFE_E_SIZE beyond).  `out` may not be NULL. */
int ife_signed_distance_map(ife_ctx *ctx, const void *mask, int mask_dtype,
                            const ife_volume_desc *vol, int inside_is_positive, int squared,
                            double *out, int mem);
/* expectedDistanceFromCenterToInterestPoint (same header, :9-43): the mean over the foreground
 * of (unsquared, inside-positive map) * prob; 0 when the mask is empty (:41).  The map is not
 * stored: the last pass feeds a reduction with a fixed partition and order (same input, same
 * bits).  prob follows `mem`; result and n_inside (the number of foreground voxels; may be NULL)
 * are HOST scalars; the call blocks. */
int ife_expected_distance(ife_ctx *ctx, const void *mask, int mask_dtype, const double *prob,
                          const ife_volume_desc *vol, double *result, int64_t *n_inside, int mem);

/* ---- resampling onto a target grid (tools/Resample.cxx:83-99) ------------------------------ *
 *
 * itk::ResampleImageFilter with an itk::TranslationTransform, linear or nearest-neighbour
 * interpolation.  Parity with ITK is unpinned (ITK's index-from-point matrix comes out of an SVD
 * inverse and its scan-line shortcut differs between versions); the arithmetic below is this
 * library's own and is normative.  Direction cosines are ignored, as on the whole hot path:
 * geometry is size, spacing and origin per axis, and the transform is axis-aligned, so everything
 * about an output voxel's position factors per axis.  All arithmetic is in double and every
 * operation rounds on its own.
 *
 * Per axis, for output index i in [0, n_t), with the source axis (n_s, s_s, O_s), the output axis
 * (n_t, s_t, O_t) and the translation T:
 *   p = O_t + (double)i * s_t             output point
 *   q = p + T                             TranslationTransform: point + offset
 *   c = (q - O_s) / s_s                   continuous index in the source
 *   inside = (c >= -0.5) && (c < (n_s - 1) + 0.5)        a NaN compares false: outside
 * and only where inside (nothing outside is ever converted to an integer):
 *   b = floor(c); if (b < 0) b = 0        c in [-0.5, 0) gives b = 0 and t < 0
 *   t = c - (double)b
 *   skip = (t <= 0) || (b + 1 > n_s - 1)
 *   near = min(floor(c + 0.5), n_s - 1)   the min bounds memory: n_s = 1, c = nextafter(0.5, 0)
 * A voxel is inside when all three axes are; every other voxel gets default_value.
 *
 * IFE_INTERP_LINEAR: with L(a, b, t, skip) = skip ? a : a + (b - a) * t -- a select, so a skipped
 * axis hands `a` on untouched (infinities, NaN payloads) and never reads the upper neighbour --
 * and v000 the source voxel at (b_x, b_y, b_z), nested x, then y, then z:
 *   vx00 = L(v000, v100, t_x, skip_x)     likewise vx10, vx01, vx11
 *   vxy0 = L(vx00, vx10, t_y, skip_y)     vxy1 = L(vx01, vx11, t_y, skip_y)
 *   v    = L(vxy0, vxy1, t_z, skip_z)
 * (the nesting of itk::LinearInterpolateImageFunction::EvaluateOptimized in three dimensions,
 * its early exits "distance <= 0" and "neighbour beyond the end index" as the skip rule).  Within
 * half a voxel of the border the edge value is extended.
 * IFE_INTERP_NEAREST: the source voxel at (near_x, near_y, near_z).
 *
 * A grid resampled onto itself comes back bit for bit where spacing and origin are dyadic; with a
 * spacing such as 0.7, c is i +- a few ulp and a voxel may come out as
 * v[i-1] + (v[i] - v[i-1]) * (1 - eps) (relative difference about 1e-13 on random data).  The
 * 2^-26 truncation with which old ITK hid this is not reproduced.
 *
 * ife_resample reads IFE_F32, IFE_I16, IFE_U8 and IFE_U16.  Linear writes float: the value is
 * formed in double and rounded once.  Nearest writes the source's own type (labels stay labels).
 * ife_resample_f64 is double in, double out (the reference tool's pixel type).
 * Refused with IFE_E_ARG before anything is written: a null pointer; an unknown dtype or
 * interpolation; a non-finite origin, translation or default value; a default value that is not
 * exactly a value of the output type; IFE_MEM_DEVICE pointers not aligned to their element size;
 * source and output ranges that overlap; a spacing that is not positive.  IFE_E_SIZE: a
 * non-positive size.  Source axes of length 1 are legal (every voxel skips that axis).  Origins,
 * the translation and the descriptors are HOST arrays; src and out follow `mem`.  Runs on the
 * context's stream; one device. */
typedef enum { IFE_INTERP_LINEAR = 0, IFE_INTERP_NEAREST = 1 } ife_interp;

int ife_resample(ife_ctx *ctx, const void *src, int src_dtype, const ife_volume_desc *src_vol,
                 const double src_origin[3], const ife_volume_desc *dst_vol,
                 const double dst_origin[3], const double translation[3], int interpolation,
                 double default_value, void *out, int mem);

int ife_resample_f64(ife_ctx *ctx, const double *src, const ife_volume_desc *src_vol,
                     const double src_origin[3], const ife_volume_desc *dst_vol,
                     const double dst_origin[3], const double translation[3], int interpolation,
                     double default_value, double *out, int mem);

/* ---- B-spline resampling, orders 0 to 5, and the 8-bit window (tools/ExtractWindow.cxx) ------ *
 *
 * itk::BSplineInterpolateImageFunction behind itk::ResampleImageFilter, then
 * itk::IntensityWindowingImageFilter.  Parity with ITK is unpinned, as for ife_resample; the
 * arithmetic below is normative.  It follows ITK's BSplineDecompositionImageFilter and
 * BSplineInterpolateImageFunction except where marked "ours".  Everything is in double and every
 * operation rounds on its own.
 *
 * Poles z (computed on the host) and horizons h = ceil(log(1e-10) / log|z|):
 *   order 2: sqrt(8)-3                                                        h = 14
 *   order 3: sqrt(3)-2                                                        h = 18
 *   order 4: sqrt(664-sqrt(438976))+sqrt(304)-19, sqrt(664+sqrt(438976))-sqrt(304)-19    h = 23, 6
 *   order 5: sqrt(135/2-sqrt(17745/4))+sqrt(105/4)-13/2,
 *            sqrt(135/2+sqrt(17745/4))-sqrt(105/4)-13/2                       h = 28, 8
 * Orders 0 and 1 have no poles: the coefficients are the source converted to double.
 *
 * Prefilter: the axes run x, then y, then z, each pass in place.  A line of length N = 1 is left
 * untouched (no gain).  Otherwise, per line c[0 .. N-1]:
 *   g = 1; for each pole z: g = g*(1-z)*(1-1/z);   c[n] = c[n]*g for every n
 *   then for each pole z, in the order above:
 *     causal start, h < N:   zn = z; s = c[0]; for n = 1..h-1: { s = s + zn*c[n]; zn = zn*z; }
 *                            c[0] = s
 *     causal start, h >= N:  zn = z; iz = 1/z; z2n = z^(N-1), formed by N-2 successive
 *                            multiplications by z starting from z (ours: no pow());
 *                            s = c[0] + z2n*c[N-1]; z2n = z2n*(z2n*iz);
 *                            for n = 1..N-2: { s = s + (zn+z2n)*c[n]; zn = zn*z; z2n = z2n*iz; }
 *                            c[0] = s/(1 - zn*zn)
 *     causal sweep:          for n = 1..N-1: c[n] = c[n] + z*c[n-1]
 *     anticausal start:      c[N-1] = (z/(z*z-1)) * (z*c[N-2] + c[N-1])
 *     anticausal sweep:      for n = N-2..0: c[n] = z*(c[n+1] - c[n])
 * The multipliers and the divisor depend on (z, N) only and come from the host; the sequence of
 * operations on the samples is the one above.
 *
 * Gather.  Per axis p, q, c and inside are exactly those of ife_resample; a voxel is inside when
 * all three axes are.  The support of an inside index starts at
 *   i0 = floor(c) - order/2 (odd orders),  floor(c + 0.5) - order/2 (even orders)
 * (integer division), its taps are i0 .. i0+order, and with w = c - (double)(i0 + order/2) the
 * weights are ITK's closed forms (left to right as written):
 *   0: [1]        1: [1-w, w]
 *   2: w1 = 0.75 - w*w; w2 = 0.5*(w - w1 + 1); w0 = 1 - w1 - w2
 *   3: w3 = (1/6)*w*w*w; w0 = 1/6 + 0.5*w*(w-1) - w3; w2 = w + w0 - 2*w3; w1 = 1 - w0 - w2 - w3
 *   4: w2_ = w*w; t = (1/6)*w2_; w0 = 0.5 - w; w0 = w0*w0; w0 = w0*((1/24)*w0);
 *      t0 = w*(t - 11/24); t1 = 19/96 + w2_*(0.25 - t); w1 = t1 + t0; w3 = t1 - t0;
 *      w4 = w0 + t0 + 0.5*w; w2 = 1 - w0 - w1 - w3 - w4
 *   5: w2_ = w*w; w5 = (1/120)*w*w2_*w2_; w2_ = w2_ - w; w4_ = w2_*w2_; w = w - 0.5;
 *      t = w2_*(w2_ - 3); w0 = (1/24)*(1/5 + w2_ + w4_) - w5;
 *      t0 = (1/24)*(w2_*(w2_ - 5) + 46/5); t1 = (-1/12)*w*(t + 4); w2 = t0 + t1; w3 = t0 - t1;
 *      t0 = (1/16)*(9/5 - t); t1 = (1/24)*w*(w4_ - w2_ - 5); w1 = t0 + t1; w4 = t0 - t1
 * Tap indices are mirrored: P = 2n-2; i = |i| mod P; if (i >= n) i = P - i.  A source axis of
 * length 1 is absent (ours): one tap, index 0, weight exactly 1.0, so that a volume with nz = 1
 * behaves as a 2-D image.  The value is the nested sum x, then y, then z (ours; ITK's flat sum
 * costs twice the multiplications), each sum starting from its first product:
 *   r(j,k) = sum_i wx[i]*coef[..];  s(k) = sum_j wy[j]*r(j,k);  v = sum_k wz[k]*s(k)
 * The float output rounds once; values beyond +-FLT_MAX clamp to +-FLT_MAX.
 * Outside voxels: extrapolate = 0 gives default_value; extrapolate = 1 gives the SOURCE voxel (not
 * the coefficient) at the clamped index per axis
 *   e = (c >= n-1) ? n-1 : (c > 0 ? min(floor(c + 0.5), n-1) : 0)
 * decided in double before any conversion (a NaN falls to 0).
 * Non-finite source samples are legal and unspecified: they spread along their lines.
 *
 * ife_resample_bspline* build their coefficients in a workspace the context owns, 8 bytes per
 * source voxel.  Refused as ife_resample refuses, before anything is written, and also with
 * IFE_E_ARG: an order outside 0..5; an extrapolate outside {0, 1}.  coef may equal src in
 * ife_bspline_coefficients_f64, which then runs in place; any other overlap is refused.
 *
 * ife_window_u8: scale = ((double)out_max - (double)out_min)/(window_max - window_min);
 * shift = (double)out_min - window_min*scale; v < window_min gives out_min, v > window_max gives
 * out_max, otherwise y = v*scale + shift, clamped to [0, 255], then truncated.  A NaN gives
 * out_min (ours).  With a mask the result is mask[i] != 0 ? result : 0.  IFE_E_ARG:
 * window_max <= window_min or either not finite; a null src or out; overlap of an input with the
 * output.  IFE_E_SIZE: n <= 0.  One device, the context's stream. */
int ife_bspline_coefficients(ife_ctx *ctx, const void *src, int src_dtype, const ife_volume_desc *vol,
                             int order, double *coef, int mem);

int ife_bspline_coefficients_f64(ife_ctx *ctx, const double *src, const ife_volume_desc *vol,
                                 int order, double *coef, int mem);

int ife_resample_bspline(ife_ctx *ctx, const void *src, int src_dtype, const ife_volume_desc *src_vol,
                         const double src_origin[3], const ife_volume_desc *dst_vol,
                         const double dst_origin[3], const double translation[3], int order,
                         int extrapolate, double default_value, float *out, int mem);

int ife_resample_bspline_f64(ife_ctx *ctx, const double *src, const ife_volume_desc *src_vol,
                             const double src_origin[3], const ife_volume_desc *dst_vol,
                             const double dst_origin[3], const double translation[3], int order,
                             int extrapolate, double default_value, double *out, int mem);

int ife_window_u8(ife_ctx *ctx, const double *src, const double *mask, int64_t n, double window_min,
                  double window_max, uint8_t out_min, uint8_t out_max, uint8_t *out, int mem);

/* ---- regions: mask bounding box, crop / pad / flip, label sets ------------------------------- *
 *
 * The preprocessing of tools/ExtractBoundingBox.cxx, ExtractMaskedRegion.cxx, ExtractSlices.cxx
 * and PadImage.cxx.  Everything here moves or counts whole elements: there is no arithmetic on
 * values, and results are exact.  One device, the context's stream; every call blocks.
 *
 * ife_mask_bounding_box: box = {x0, y0, z0, sx, sy, sz}, the tightest box around the foreground
 * of `mask` (dense, x fastest), and *count, the number of foreground voxels.  box and count are
 * HOST pointers whatever mem is.  mask_dtype: IFE_U8, IFE_U16, IFE_I16 or IFE_F32.  An integer
 * element is foreground when it is != 0 (a uint16 of 256 is foreground); a float when its bit
 * pattern is anything but +-0, (bits & 0x7fffffff) != 0, so that denormals and NaN are foreground
 * whatever the denormal mode of a compare is.  An empty mask gives IFE_OK, six zeros and count 0.
 * [ITK-upstream, parity unpinned] this is what ImageMaskSpatialObject<3>::
 * GetAxisAlignedBoundingBoxRegion returns, and the union of the component boxes that
 * ExtractSlices.cxx:123-155 builds.
 *
 * ife_extract_region: a copy of bits, no conversion; elem_bytes is 1, 2, 4 or 8.  region =
 * {ix, iy, iz, sx, sy, sz} in the source's index space, sizes >= 1; the index may be negative and
 * the box may reach beyond the source or lie wholly outside it.  dst is a dense volume of
 * sx * sy * sz elements, x fastest, and
 *   dst[x, y, z] = S(ix + fx(x), iy + fy(y), iz + fz(z))
 *   fa(i) = size_a - 1 - i where bit a of flip (0 .. 7) is set, else i
 *   S = the source inside [0, n) on every axis, elsewhere the elem_bytes bytes at the HOST pointer
 *       pad_value.
 * pad_value may be NULL only when the region lies inside the source.  This covers
 * itk::ExtractImageFilter and RegionOfInterestImageFilter (region inside the source),
 * ConstantPadImageFilter (index -lower, size n + lower + upper) and FlipImageFilter.  src_mem and
 * dst_mem are independent, so that a volume uploaded once serves many fetches to the host.
 * IFE_E_ARG: elem_bytes not 1, 2, 4 or 8; a size below 1; flip outside 0 .. 7; a NULL pad_value
 * with a region that reaches outside; a null src, dst or region; a DEVICE pointer not aligned to
 * elem_bytes; DEVICE src and dst ranges that overlap.  IFE_E_SIZE: a region of more than 2^40
 * bytes, or a voxel count that overflows.
 *
 * ife_label_membership: out[i] = inside where labels[i] occurs in include[0 .. n_include), else
 * outside (the functor of ExtractMaskedRegion.cxx:62-67).  labels_dtype is IFE_U8 or IFE_U16 and
 * out has the same type.  include needs no order and may repeat values; n_include == 0 makes
 * every element outside.  IFE_E_ARG: an include, inside or outside value outside the dtype's
 * range; a null pointer; DEVICE labels and out that overlap.  IFE_E_SIZE: n <= 0 or n > 2^40. */
int ife_mask_bounding_box(ife_ctx *ctx, const void *mask, int mask_dtype, const ife_volume_desc *vol,
                          int64_t box[6], int64_t *count, int mem);

int ife_extract_region(ife_ctx *ctx, const void *src, int elem_bytes, const ife_volume_desc *src_vol,
                       const int64_t region[6], int flip, const void *pad_value, void *dst, int src_mem,
                       int dst_mem);

int ife_label_membership(ife_ctx *ctx, const void *labels, int labels_dtype, int64_t n, const int *include,
                         int n_include, int inside, int outside, void *out, int mem);

/* Device buffers for callers without a HIP runtime of their own (the host tools: ExtractSlices
 * uploads its volume once and fetches every slice from it).  ife_device_alloc gives `bytes` bytes
 * on the context's device, aligned to at least 256; ife_device_upload copies host bytes into such a
 * buffer on the context's stream and waits; ife_device_free takes a pointer of ife_device_alloc
 * (NULL is allowed) and waits for the stream first.  IFE_E_ARG: a null pointer, bytes == 0. */
int ife_device_alloc(ife_ctx *ctx, size_t bytes, void **ptr);
int ife_device_upload(ife_ctx *ctx, void *dst, const void *src, size_t bytes);
int ife_device_free(ife_ctx *ctx, void *ptr);

/* ---- sampling: seeded draws of mask voxels and boxes, a batched box gather --------------------- *
 *
 * The random steps of tools/GenerateROIs.cxx, GenerateROIsManyRegions.cxx, MakeBag.cxx (through
 * ROI/RegionOfInterestGenerator.hxx:22-62) and DetermineHistogramBinEdges_MultiScaleEigenvalue
 * Features.cxx:112-133, without the mask on the host, and the gather of tools/SampleROIs.cxx:151-167.
 * The reference seeds its generators from the clock, so there is nothing to be equal to: the draw
 * is defined here, and the device is held equal to tests/sampling_oracle.py's restatement of it.
 * Integers only; results are exact.  One device, the context's stream; every call blocks.
 *
 * Volume and mask.  The volume is dense, x fastest, with at most 2^32-1 voxels (IFE_E_SIZE beyond,
 * as for the dense calls).  mask_dtype is IFE_U8 or IFE_U16.  size = {sx, sy, sz}, each >= 1; NULL
 * means {1, 1, 1}.  h = size / 2 by integer division (an even size is off-centre, as in
 * ROI/DenseROIGenerator.hxx:35-40).  Voxel (x, y, z) fits when the box [x - hx, x - hx + sx) x
 * [y - hy, ...) x [z - hz, ...) lies inside the volume.
 *
 * Sets.  values is a HOST array of n_values entries, 0 <= n_values <= 32.
 *   n_values == 0:  one set, mask != 0
 *   per_value == 0: one set, mask in values[0 .. n_values)
 *   per_value == 1: n_values sets, set j is mask == values[j]; a repeated value is a set of its own
 * A_j: the voxels of set j that fit, in increasing linear index x + nx * (y + ny * z); N_j = |A_j|.
 *
 * Draw k of set j, k = first_draw + i for 0 <= i < n_draws, taken as an unsigned 64-bit number:
 *   o = Philox4x32-10(counter = (k mod 2^32, k >> 32, (stream + j) mod 2^32, 0),
 *                     key = (seed mod 2^32, seed >> 32))
 *   u = o[0] + 2^32 * o[1]
 *   r = floor(u * N_j / 2^64)          the high word of the 64 x 64 bit product
 *   the result is A_j[r]
 * Uniform over the admissible voxels, with replacement, as the reference's rejection loop is; the
 * bias of the multiply-shift is below N_j / 2^64.  Philox4x32-10 is the published function
 * (Salmon et al., SC11): multipliers 0xD2511F53 (on word 0) and 0xCD9E8D57 (on word 2), key
 * increments 0x9E3779B9 and 0xBB67AE85 after each of the first nine rounds, a round
 *   c <- (hi(M1 * c2) ^ c1 ^ k0, lo(M1 * c2), hi(M0 * c0) ^ c3 ^ k1, lo(M0 * c0)).
 * Counter and key all zero give 6627e8d5 e169c58d bc57ac4c 9b00dbd8.  A draw depends on (seed,
 * stream + j, k) and the mask alone: draws [0, 100) are draws [0, 40) followed by [40, 100).
 *
 * ife_sample_positions: positions[set][i] = the linear index of the draw.  ife_random_rois:
 * rois[set][i] = {x - hx, y - hy, z - hz, sx, sy, sz} of the drawn voxel (x, y, z).  mask and the
 * output follow mem; n_admissible is a HOST array of one entry per set and receives N_j.
 * n_draws == 0 with a NULL output is legal and gives the counts alone.  Where some N_j == 0 and
 * n_draws > 0 the call writes n_admissible, returns IFE_E_ARG with a message that names the set
 * and writes nothing else (the reference would draw forever).  IFE_E_ARG also: a value outside the
 * dtype's range, per_value with n_values == 0, n_values outside 0 .. 32, a size below 1, a
 * negative count, a null pointer, a DEVICE pointer not aligned to its element size.  IFE_E_SIZE:
 * more than 2^36 draws over all sets.
 *
 * ife_extract_rois: dst[r][z][y][x] = src[rois[r].z0 + z][rois[r].y0 + y][rois[r].x0 + x], a copy
 * of bits of elements of 1, 2, 4 or 8 bytes; rois = [n_rois][6] as above; src, rois and dst follow
 * mem.  All boxes must have the size of the first, at least 1, and lie inside the volume, else
 * IFE_E_ARG with dst untouched; DEVICE boxes are checked on the device before anything reads
 * through them.  n_rois == 0 is IFE_OK.  IFE_E_SIZE: more than 2^40 bytes of output. */
int ife_sample_positions(ife_ctx *ctx, const void *mask, int mask_dtype, const ife_volume_desc *vol,
                         const int *values, int n_values, int per_value, const int64_t *size, uint64_t seed,
                         uint32_t stream, uint64_t first_draw, int64_t n_draws, int64_t *positions,
                         int64_t *n_admissible, int mem);

int ife_random_rois(ife_ctx *ctx, const void *mask, int mask_dtype, const ife_volume_desc *vol, const int *values,
                    int n_values, int per_value, const int64_t *size, uint64_t seed, uint32_t stream,
                    uint64_t first_draw, int64_t n_draws, int64_t *rois, int64_t *n_admissible, int mem);

int ife_extract_rois(ife_ctx *ctx, const void *src, int elem_bytes, const ife_volume_desc *vol, const int64_t *rois,
                     int64_t n_rois, void *dst, int mem);

/* ---- census and coverage: the two questions of tools/ImageBrowser.cxx ---------------------------- *
 *
 * Which values occur in a volume and how often (its `s` command, :165-186), and how many random
 * boxes it takes to cover the region between two thresholds (its `r` command, :24-100).  Integers
 * only; results are exact.  One device, the context's stream; every call blocks.
 *
 * ife_value_census_f32: the distinct values of values[0 .. n) in ascending order in uniq, and in
 * counts how often each occurs: the std::set<float> of :165-168 and the DenseHistogram over its
 * values of :169-173, whose bin i = (uniq[i-1], uniq[i]] counts the elements equal to uniq[i] and
 * whose trailing bin (uniq[last], inf) is always 0 and is not written.  Stated on bit patterns, so
 * that no compare's denormal mode matters:
 *   NaN       (bits & 0x7fffffff) > 0x7f800000.  NaNs are left out and counted in *n_nan (the
 *             reference's set has no defined behaviour there: a departure)
 *   zeros     -0 and +0 are one value, reported as +0.0 (the reference reports whichever comes first
 *             in raster order: a departure)
 *   others    two elements are the same value iff their bits are equal; uniq ascends in float
 *             order; denormals are values of their own; -inf and +inf are ordinary values
 * uniq and counts (capacity entries each) follow mem; n_unique and n_nan are HOST pointers.
 * capacity == 0 with uniq == counts == NULL is legal and gives the two counts alone.  Where
 * *n_unique > capacity the call writes n_unique and n_nan, returns IFE_E_ARG with a message that
 * names both numbers and writes nothing else.  Workspace of the context: a sorted copy and the
 * sort's partner, 4 bytes per element each, and one count per 256 elements.  IFE_E_ARG also: a null
 * pointer, n <= 0, a negative capacity, a DEVICE pointer not aligned to its element.  IFE_E_SIZE:
 * n > 2^32-1; the sort underneath takes 2^31-1 elements and anything beyond is refused likewise.
 *
 * ife_threshold_mask: mask[i] = 1 where low <= image[i] <= high, else 0, both ends inclusive:
 * itk::BinaryThresholdImageFilter with inside 1 and outside 0, as :35-42 sets it.  NaN elements give
 * 0; -0 equals +0; the decision is taken on the order-preserving integer image of the bits, so
 * denormal bounds and values compare as IEEE 754 says whatever the kernel's denormal mode.  image
 * and mask follow mem; count is a HOST pointer, may be NULL, and receives the number of ones
 * (regionSize, :61-66).  IFE_E_ARG: low > high (ITK throws there), a NaN bound, a null image or
 * mask, a DEVICE image not aligned to its element, DEVICE image and mask ranges that overlap.
 * IFE_E_SIZE: n <= 0 or n > 2^40.
 *
 * ife_roi_coverage: with V_r the union of the boxes k < round_ends[r],
 *   visited[r]   = |V_r|
 *   hits[r]      = |V_r and {mask != 0}|
 *   *region_size = |{mask != 0}|
 * the three numbers of every line :72-99 prints; the rounds are cumulative.  The volume is dense,
 * x fastest, with at most 2^32-1 voxels (IFE_E_SIZE beyond).  mask_dtype is IFE_U8 or IFE_U16 and
 * foreground is != 0 (a uint16 of 256 is foreground).  rois = [n_rois][6] {x0, y0, z0, sx, sy, sz};
 * the boxes may differ in size.  mask and rois follow mem.  round_ends is a HOST array of n_rounds
 * entries, 1 <= n_rounds <= 64, non-decreasing, 0 <= round_ends[r] <= n_rois.  visited and hits
 * (HOST, n_rounds entries each) and region_size (HOST, may be NULL) receive the counts.  n_rois ==
 * 0 (rois may be NULL then) or a round end of 0 gives zeros.  A box with a size below 1 or that
 * leaves the volume is IFE_E_ARG with nothing written; DEVICE boxes are checked on the device
 * before anything is painted.  IFE_E_ARG also: a decreasing round_ends, an end beyond n_rois,
 * n_rounds outside 1 .. 64, a null pointer, a DEVICE pointer not aligned to its element.
 * Workspace of the context: two planes of one bit per voxel. */
int ife_value_census_f32(ife_ctx *ctx, const float *values, int64_t n, float *uniq, uint32_t *counts,
                         int64_t capacity, int64_t *n_unique, int64_t *n_nan, int mem);

int ife_threshold_mask(ife_ctx *ctx, const float *image, int64_t n, float low, float high, uint8_t *mask,
                       int64_t *count, int mem);

int ife_roi_coverage(ife_ctx *ctx, const void *mask, int mask_dtype, const ife_volume_desc *vol, const int64_t *rois,
                     int64_t n_rois, const int64_t *round_ends, int n_rounds, int64_t *visited, int64_t *hits,
                     int64_t *region_size, int mem);

/* ---- scale selection: the maximum over scales of a gamma-normalised measure -------------------- *
 *
 * Ours: the reference computes its features per scale and never reduces over scales (SURVEY.md
 * section 0.6).  For every voxel and every requested measure the call gives the largest response
 * over the scales and the index of the scale that reached it, without ever holding more than one
 * scale of features: 5 bytes per voxel and measure leave the device instead of 32 per voxel and
 * scale.
 *
 * Per voxel and scale s:
 *   e1, e2, e3   feature components 2, 3, 4 (|e1| >= |e2| >= |e3|) and L component 5, exactly what
 *                ife_emphysema_features gives for sigmas[s] -- with IFE_OPT_DIFFERENTIAL at 1, what
 *                ife_differential_features gives
 *   w_s          (float)pow((double)sigmas[s], 2 * (double)gamma), formed on the host
 *   a1 = w_s*e3, a2 = w_s*e2, a3 = w_s*e1, in float: |a1| <= |a2| <= |a3|
 *   polarity     +1: bright structures (negative curvature), -1: dark ones; a_k "has the sign"
 *                when -polarity * a_k > 0
 *   Ra2 = a2^2 / a3^2;  Rb2 = a1^2 / |a2*a3|, 0 where a2 == 0;  S2 = a1^2 + a2^2 + a3^2
 *   A = exp(-Ra2 / (2 alpha^2));  B = exp(-Rb2 / (2 beta^2));  C = 1 - exp(-S2 / (2 c^2))
 *   in float arithmetic with expf; the three reciprocals 1/(2 alpha^2), 1/(2 beta^2), 1/(2 c^2)
 *   are formed on the host in double and rounded to float.
 * The response r of a measure kind:
 *   IFE_SS_LAPLACIAN   -polarity * (w_s * L): one float product, exact (Lindeberg's blob detector)
 *   IFE_SS_TUBE        (1 - A) * B * C        where a2 and a3 have the sign, else 0
 *   IFE_SS_PLATE       A * B * C              where a3 has the sign, else 0
 *   IFE_SS_BLOB        (1 - A) * (1 - B) * C  where a1, a2 and a3 have the sign, else 0
 * The fold over the scales, in the order given: best = 0 and index = 255; scale s replaces them
 * only when r > best, strictly, so the first of equal scales wins and a NaN never does.  A voxel
 * outside the mask has zero features, hence (0, 255).
 *
 * measures and sigmas are HOST arrays; image, mask, response and scale_index follow mem (HOST or
 * DEVICE; the call blocks in both).  response is [n_measures][nvox] float, scale_index the same
 * in uint8 or NULL, which changes nothing in response.  DEVICE: response at any float alignment,
 * scale_index at any byte.  Volume, sigmas, image and mask as for ife_emphysema_features.
 * IFE_E_ARG with a message that names the argument: n_measures outside 1 .. IFE_SS_MAX_MEASURES;
 * n_sigmas > 255; an unknown kind; a polarity other than +1 or -1; gamma negative or not finite;
 * alpha, beta or c not positive and finite for the three Frangi kinds (IFE_SS_LAPLACIAN ignores
 * them).  A refused call writes nothing and leaves the context usable.  Workspace of the
 * context: that of the feature call and one planar scale of features, 32 bytes per voxel. */
typedef enum { IFE_SS_LAPLACIAN = 0, IFE_SS_TUBE = 1, IFE_SS_PLATE = 2, IFE_SS_BLOB = 3 } ife_scale_measure_kind;
#define IFE_SS_MAX_MEASURES 4
typedef struct ife_scale_measure {
  int32_t kind, polarity;
  float gamma, alpha, beta, c;
} ife_scale_measure;

int ife_scale_select(ife_ctx *ctx, const void *image, int image_dtype, const void *mask, int mask_dtype,
                     const ife_volume_desc *vol, const float *sigmas, int n_sigmas,
                     const ife_scale_measure *measures, int n_measures, float *response, uint8_t *scale_index,
                     int mem);

/* ---- measurement ------------------------------------------------------------------- */

#define IFE_MAX_KERNEL_KINDS 24
typedef struct {
  char name[48];
  int64_t launches;
  double total_ms; /* sum of hipEvent elapsed times */
} ife_kernel_time;
/* With IFE_OPT_PROFILE=1: per-kernel-kind device time accumulated since the last
 * ife_reset_kernel_times.  Synchronises the stream.  Returns the number of entries
 * written (<= max_entries) or a negative status. */
int ife_get_kernel_times(ife_ctx *ctx, ife_kernel_time *entries, int max_entries);
int ife_reset_kernel_times(ife_ctx *ctx);
/* The box's streaming rate with 16-byte accesses per lane (no reference counterpart; bench.py
 * prints it beside the 8 TB/s peak): mode 0 writes `bytes` to dst (a fill), mode 1 copies
 * `bytes` from src to dst; DEVICE pointers, 16-byte aligned.  One warm pass, then `reps`
 * timed passes between hipEvents on the context's stream; *ms_per_pass is their average. */
int ife_measure_stream(ife_ctx *ctx, int mode, void *dst, const void *src, size_t bytes, int reps,
                       double *ms_per_pass);

#ifdef __cplusplus
}
#endif
#endif /* IFE_HIP_H */
