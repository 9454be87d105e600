/*
 * itermvs_hip.h -- C ABI of libitermvs_hip.so (hand-written gfx950 HIP kernels for the
 * IterMVS matching hot path).
 *
 * The reference (FangjinhuaWang/IterMVS) has NO native / FFI interface: its hot path is
 * Python calling stock PyTorch ops.  The entry points below are therefore the seams of the
 * reference's Python functions, lowered to plain pointers + sizes; each one cites the
 * reference code it replaces (paths relative to the reference repository).  The ctypes
 * binding a maintainer of the reference would add is shown in INTEGRATION.md and lives in
 * itermvs_amd/_lib.py.
 *
 * Conventions:
 *   - every function ENQUEUES work on `stream` and returns immediately: no allocation, no
 *     synchronisation, no global mutable state (re-entrant across streams / threads);
 *   - all tensors are caller-owned DEVICE buffers of fp32 unless stated, borrowed for the
 *     duration of the enqueue; inputs are never written;
 *   - return value 0 = ok, negative = itermvs_status (bad dims, null pointer, unsupported
 *     channel count, misalignment); nothing is thrown;
 *   - `void* stream` is a hipStream_t (NULL = default stream).
 */
#ifndef ITERMVS_HIP_H
#define ITERMVS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the prototypes of this header are its ONLY dynamic symbols
 * (tests/test_host_cpu.py holds `nm -D` to that). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define ITERMVS_ABI_VERSION 20
#define ITERMVS_MAX_SRC 16     /* source views per reference view (pair.txt holds 10) */
#define ITERMVS_MAX_HYP 8      /* hypotheses per level in the iteration branch (4,4,2) */
#define ITERMVS_GROUPS 8       /* models/itermvs.py:28  */
#define ITERMVS_PROB_BINS 256  /* models/itermvs.py:134 */
#define ITERMVS_WINDOW_RADIUS 4 /* models/itermvs.py:135 */

typedef enum itermvs_status {
    ITERMVS_OK = 0,
    ITERMVS_ERR_NULL = -1,        /* required pointer is NULL                     */
    ITERMVS_ERR_DIMS = -2,        /* non-positive / inconsistent dimension        */
    ITERMVS_ERR_CHANNELS = -3,    /* C not in {16,32,48} (C/G must be 2,4,6)      */
    ITERMVS_ERR_VIEWS = -4,       /* S < 1 or S > ITERMVS_MAX_SRC                 */
    ITERMVS_ERR_ALIGN = -5,       /* pointer / stride not aligned for vector path */
    ITERMVS_ERR_LAYOUT = -6,      /* fused kernels need channels-last features    */
    ITERMVS_ERR_LAUNCH = -7,      /* hipLaunchKernel failed (see hipGetLastError) */
    ITERMVS_ERR_DTYPE = -8,       /* feature storage type not supported by this entry point */
    ITERMVS_ERR_MODEL = -9        /* camera model not supported by itermvs_undistort_rgb8 (FOV, THIN_PRISM_FISHEYE, unknown id) */
} itermvs_status;

/* Storage type of FEATURE maps (the pyramids the correlation kernels gather from).  Arithmetic is always fp32: 16-bit
 * storage halves the gathered bytes (BASELINE cfg 4 "bf16", cfg 5 "fp16"); coordinates, depths, view weights, correlations
 * and every other tensor stay fp32. */
typedef enum itermvs_dtype {
    ITERMVS_F32 = 0,
    ITERMVS_F16 = 1,              /* IEEE binary16 */
    ITERMVS_BF16 = 2              /* bfloat16      */
} itermvs_dtype;

/* library / ABI identification */
int itermvs_version(void);
const char* itermvs_error_string(int status);

/* A 4-D feature map addressed with ELEMENT strides, so NCHW and channels-last (NHWC) views
 * of torch tensors are both accepted.  The fused kernels require sc == 1 (channels-last). */
typedef struct itermvs_fmap {
    const void* data;         /* elements of `dtype` */
    int64_t sb, sc, sy, sx;   /* strides of batch, channel, row, column (elements) */
    int32_t C, H, W;
    int32_t dtype;            /* itermvs_dtype; 16-bit storage is accepted by the fused correlation entry points and
                                 itermvs_ref_quarter, everything else takes ITERMVS_F32 */
} itermvs_fmap;

/* The S source-view feature maps of one pyramid level: per-view base pointers sharing one
 * set of element strides (views of a [B,V,...] tensor or separately allocated maps). */
typedef struct itermvs_level_src {
    const void* view[ITERMVS_MAX_SRC];   /* elements of `dtype` */
    int64_t sb, sc, sy, sx;
    int32_t C, H, W;
    int32_t dtype;                       /* itermvs_dtype (all levels of one call share it) */
} itermvs_level_src;

/* ------------------------------------------------------------------------------------------
 * itermvs_compose_proj -- models/module.py:77-90
 *   proj = src_proj @ inverse(ref_proj); rot = proj[:3,:3]; trans = proj[:3,3]
 * `mats` is [n_sets, V, 4, 4] row-major (view 0 = reference); `out` is [n_sets, V-1, 12]
 * holding rows of [rot | trans].  Inverse and product are evaluated in fp64 and rounded
 * once to fp32.  `nan_flag` (device int32, may be NULL) is OR-ed with 1 when a result is
 * NaN -- the deferred form of the reference's host-side asserts (module.py:83,87).
 * When `inv_min` != NULL the same launch also writes the inverse depth range of the batch,
 * inv_min[b] = 1 / depth_min[b], inv_max[b] = 1 / depth_max[b] (models/itermvs.py:240-241), b < B.
 * ITERMVS_ERR_DIMS: n_sets * (V - 1) > 2^31 - 1.
 * ------------------------------------------------------------------------------------------ */
int itermvs_compose_proj(const float* mats, int32_t n_sets, int32_t V, float* out,
                         int32_t* nan_flag, const float* depth_min, const float* depth_max,
                         int32_t B, float* inv_min, float* inv_max, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_warp -- models/module.py:68-125  differentiable_warping(src_fea, src_proj,
 *   ref_proj, depth_samples, return_mask)
 * Plain (un-fused) seam: writes the warped volume out[B,C,N,H,W] (contiguous) and, when
 * `mask` != NULL, the validity mask [B,N,H,W] as uint8.  `proj` = [B,12] from
 * itermvs_compose_proj.  Any strides / any C.  Kept for API completeness and unit tests;
 * the engine itself never materialises the warped volume.
 * Limits of the one-thread-per-item launches (here and below; ITERMVS_ERR_DIMS before any launch): the item count of a
 * 256-thread launch is at most 2^32 - 256 (gridDim.x * blockDim.x < 2^32), a batch or view count carried in grid.y at most
 * 65535, and 2^31 - 1 items where the kernel indexes in 32 bits.  Here: B * N * H * W <= 2^32 - 256.
 * ------------------------------------------------------------------------------------------ */
int itermvs_warp(const itermvs_fmap* src, const float* proj, const float* depth,
                 int32_t B, int32_t N, int32_t H, int32_t W, float* out, uint8_t* mask,
                 void* stream);

/* gradient of itermvs_warp w.r.t. src (grid math is no_grad in the reference, module.py:77):
 * grad_src[B,C,H1,W1] (contiguous NCHW, must be zero-filled) += scatter of grad_out[B,C,N,H,W]
 * B * N * H * W <= 2^32 - 256, H1 * W1 <= 2^31 - 1. */
int itermvs_warp_backward(const float* grad_out, const float* proj, const float* depth,
                          int32_t B, int32_t C, int32_t N, int32_t H, int32_t W,
                          int32_t H1, int32_t W1, float* grad_src, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_ref_quarter -- models/itermvs.py:95-98
 * Reference-view features of the three pyramid levels resampled onto the 1/4 grid and packed
 * channels-last: out[B,H,W,C1+C2+C3] (level 1: x0.5 bilinear == 2x2 mean; level 2: copy;
 * level 3: x2 bilinear, align_corners=False).  H,W = size of level 2.
 * Any element strides; a channels-last map (sc == 1) is read four channels per load and must then have its data
 * pointer 16-byte (fp32) / 8-byte (16-bit) aligned and sx, sy, sb multiples of 4 (ITERMVS_ERR_ALIGN otherwise).
 * ------------------------------------------------------------------------------------------ */
int itermvs_ref_quarter(const itermvs_fmap* ref_l1, const itermvs_fmap* ref_l2,
                        const itermvs_fmap* ref_l3, int32_t B, float* out, void* stream);
/* itermvs_ref_quarter_compose -- itermvs_ref_quarter and, in the SAME launch (a few extra threads), itermvs_compose_proj with
 * its arguments (mats .. inv_max; Bd = batch size of the depth range): the two are independent and both precede the
 * correlation kernels. */
int itermvs_ref_quarter_compose(const itermvs_fmap* r1, const itermvs_fmap* r2, const itermvs_fmap* r3, int32_t B, float* out,
                                const float* mats, int32_t n_sets, int32_t V, float* proj_out, int32_t* nan_flag,
                                const float* depth_min, const float* depth_max, int32_t Bd, float* inv_min, float* inv_max,
                                void* stream);

/* itermvs_copy_multi -- n (<= 8) device-to-device copies of bytes[i] bytes in ONE launch: the staging of a sample (images +
 * cameras + depth range) into the static input buffers a captured hipGraph reads (engine.GraphedRunner).  src / dst / bytes
 * are HOST arrays. */
int itermvs_copy_multi(const void* const* src, void* const* dst, const int64_t* bytes, int32_t n, void* stream);

/* itermvs_box_probe -- a fixed micro-kernel for bench.py's box calibration (no reference counterpart: the reference prints
 * wall-clock only, eval.py:130-137): `blocks` workgroups of 4 waves issue `iters` x 4 independent v_mfma_f32_16x16x4_f32 per
 * wave (2*16*16*4 FLOP each) and store one float per thread to sink[blocks*256].  clocks (device, 2 x uint64, may be NULL):
 * workgroup 0 writes its shader-clock ticks (s_memtime) and its constant-rate 100 MHz ticks (s_memrealtime) across the loop
 * -> the sustained shader clock of THIS chip under matrix load.  The companion bandwidth probe is itermvs_copy_multi on a
 * 256 MB buffer.  Timed by the caller with events on `stream`. */
int itermvs_box_probe(float* sink, int32_t blocks, int32_t iters, uint64_t* clocks, void* stream);
/* itermvs_box_chase -- the latency probe of the same calibration: ONE lane follows i -> ring[i] from `start` for `steps` dependent
 * loads (ring: device uint32 indices forming one cycle, built by the caller; its size selects L2 / memory-side cache / HBM);
 * out[0] = the final index (start of the next call: untouched lines), clocks[0] = elapsed 100 MHz ticks (s_memrealtime),
 * clocks[1] = elapsed shader-clock ticks (the clock of a nearly idle chip).  clocks: 2 x uint64. */
int itermvs_box_chase(const uint32_t* ring, uint32_t start, int32_t steps, uint32_t* out, uint64_t* clocks, void* stream);
/* itermvs_clock_stamp -- out (device, uint64[16][2], zeroed by the caller): every XCD writes { its 100 MHz counter, its shader-clock
 * counter } to slot XCC_ID.  Two stamps around other work on the stream: per XCD, delta(shader) / delta(100 MHz) x 100 = the clock
 * in MHz the chip sustained under THAT work (bench.py `box.sclk_workload_MHz`). */
int itermvs_clock_stamp(uint64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_corr_iter -- models/itermvs.py:84-120 (Evaluation.forward, iteration branch, up to
 * but excluding CorrNet) fused with module.py:68-125 and, optionally, the hypothesis
 * construction of itermvs.py:290-293.
 * For every 1/4-res pixel, level l in {1,2,3}, hypothesis n, group g:
 *   out_l[b,n,g,y,x] = sum_s w[b,s,y,x] * corr_s / (1e-5 + sum_s w[b,s,y,x]),
 *   corr_s = mean_{c in group g} warp(src_l[s])[c] * ref_q[c]
 * No warped volume / cost volume is written to memory.
 * ------------------------------------------------------------------------------------------ */
typedef struct itermvs_corr_iter_params {
    int32_t B, S, H, W;                        /* sample grid = level-2 size              */
    int32_t N[3];                              /* hypotheses per level (reference: 4,4,2) */
    int32_t impl;                              /* reserved, must be 0 (one kernel form)   */
    itermvs_level_src src[3];                  /* [level-1]; channels-last (sc == 1)      */
    const float* ref_q;                        /* [B,H,W,C1+C2+C3] from itermvs_ref_quarter */
    const float* proj;                         /* [3,B,S,12] from itermvs_compose_proj    */
    const float* view_w;                       /* view weights, element (b,s,y,x) at view_w[b*view_w_sb + s*view_w_ss + (y*W+x)*view_w_sp] */
    int64_t view_w_sb, view_w_ss, view_w_sp;   /* all 0 = contiguous [B,S,H,W]; the engine stores them INTERLEAVED [B,H,W,S]
                                                * (ss = 1, sp = S): the S weights of a pixel are one vector load of a lane
                                                * quad.  itermvs_corr_iter_backward needs the contiguous form. */
    const float* depth[3];                     /* explicit hypotheses [B,N_l,H,W] or NULL */
    const float* norm_depth;                   /* normalised depth at norm_depth[b*norm_depth_sb + y*W + x]; used where depth[l] == NULL */
    int64_t norm_depth_sb;                     /* batch stride (elements) of norm_depth   */
    float offsets[3][ITERMVS_MAX_HYP];         /* normalised offsets corr_interval*interval_scale (itermvs.py:229-235) */
    const float* inv_depth_min;                /* device [B]  1/depth_min                 */
    const float* inv_depth_max;                /* device [B]  1/depth_max                 */
    float* out[3];                             /* [B,N_l,8,H,W] contiguous (CorrNet input [B*N,8,H,W]) */
} itermvs_corr_iter_params;

int itermvs_corr_iter(const itermvs_corr_iter_params* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_corr_init -- models/itermvs.py:48-51 (+ :11-19 DepthInitialization when depth==NULL)
 * Per-view group correlation at level 3 for all N hypotheses:
 *   out[b,s,n,g,y,x]  (== PixelViewWeight input [B*S*N, 8, H, W])
 * ------------------------------------------------------------------------------------------ */
typedef struct itermvs_corr_init_params {
    int32_t B, S, H, W, N;                     /* sample grid = level-3 size; N = 32      */
    int32_t out_layout;                        /* 0 = out [B,S,N,8,H,W]; 1 = groups last [B,S,N,H,W,8] (out 16-byte aligned): the layout
                                                * itermvs_conv2d (in_layout 1) stages with two 16-byte loads per pixel.  The backward takes 0 */
    itermvs_level_src src;                     /* level-3 source features, channels-last  */
    itermvs_fmap ref;                          /* level-3 reference features (any strides) */
    const float* proj;                         /* [B,S,12]                                */
    const float* depth;                        /* [B,N,H,W] or NULL (generate uniform inverse depth) */
    const float* inv_depth_min;                /* device [B] */
    const float* inv_depth_max;                /* device [B] */
    float* out;                                /* [B,S,N,8,H,W] (see out_layout) */
} itermvs_corr_init_params;

int itermvs_corr_init(const itermvs_corr_init_params* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * Slot forms of itermvs_corr_iter / itermvs_corr_init (scan mode: each image's feature pyramid is computed once and kept
 * in a per-level slab; the reference recomputes FeatureNet on all V views of every sample, models/net.py:52-65 called per
 * sample from eval.py:128-133).  The source map of (batch item b, view s) is read at
 *     slab + slot[b * S + s] * slot_stride        (elements of `dtype`)
 * so one captured graph serves every reference view: a replay refreshes the device slot table, not kernel arguments.
 * Entries outside [0, n_slots) are clamped into it (a wrong map, never memory outside the slab).  Same arithmetic and tap
 * order as the direct forms, bit for bit; the parameter block is the same, its `src` member is ignored.
 * ------------------------------------------------------------------------------------------ */
typedef struct itermvs_level_slots {
    const void* slab;                    /* slot 0; elements of `dtype`, 16-byte aligned */
    int64_t slot_stride;                 /* elements between two slots (>= H * sy)       */
    int64_t sc, sy, sx;                  /* channel (must be 1), row, column strides     */
    int32_t C, H, W;
    int32_t dtype;                       /* itermvs_dtype (all levels of one call share it) */
    int32_t n_slots;                     /* slots in the slab                            */
    const int32_t* slot;                 /* DEVICE [B,S] slot table                      */
} itermvs_level_slots;

int itermvs_corr_iter_slots(const itermvs_corr_iter_params* p, const itermvs_level_slots src[3], void* stream);
int itermvs_corr_init_slots(const itermvs_corr_init_params* p, const itermvs_level_slots* src, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_tap_indices -- diagnostic: the bilinear tap indices the FUSED kernels use (models/module.py:99-115 followed by
 * grid_sample's un-normalisation and floor, ATen GridSampler.h:31,205-207).  itermvs_corr_iter / itermvs_corr_init and
 * their gradients never store the sampling position; this entry evaluates it with the same device functions in the same
 * order (hypothesis construction, ray, projection with the library's division form, floor, bounds) and writes, for every
 * (b, view s, hypothesis n, pixel p = y*W + x) of the sample grid:
 *   out[b,s,n,0,p] = floor(ix)   out[b,s,n,1,p] = floor(iy)     as int32 (NaN -> INT32_MIN, saturated at +-2^30)
 *   out[b,s,n,2,p] = bit 0: column x0 inside the source map, bit 1: x0+1, bit 2: row y0, bit 3: y0+1
 *   coords[b,s,n,0,p] = ix, coords[b,s,n,1,p] = iy  (optional, may be NULL)
 * Hypotheses: `depth` [B,N,H,W] when given; else, with init != 0, the N initial planes (models/itermvs.py:13-17); else
 * norm_depth + offsets[n] clamped and un-normalised (models/itermvs.py:291-293, N <= ITERMVS_MAX_HYP).
 * tests/test_tap_indices_gpu.py holds it bit for bit to the reference's own sampling grids (tests/golden/tap_cases.npz).
 * ------------------------------------------------------------------------------------------ */
typedef struct itermvs_tap_params {
    int32_t B, S, H, W;                        /* sample grid                              */
    int32_t N;                                 /* hypotheses                               */
    int32_t H1, W1;                            /* source map size                          */
    int32_t init;                              /* != 0: generate the initial planes        */
    const float* proj;                         /* [B,S,12]                                 */
    const float* depth;                        /* [B,N,H,W] or NULL                        */
    const float* norm_depth;                   /* element (b,y,x) at norm_depth[b*norm_depth_sb + y*W + x] */
    int64_t norm_depth_sb;
    float offsets[ITERMVS_MAX_HYP];
    const float* inv_depth_min;                /* device [B] */
    const float* inv_depth_max;                /* device [B] */
    int32_t* out;                              /* [B,S,N,3,H,W] */
    float* coords;                             /* [B,S,N,2,H,W] or NULL */
} itermvs_tap_params;

int itermvs_tap_indices(const itermvs_tap_params* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gradients of the two fused correlation entry points for training (train.py:194-243; the training branches of
 * models/itermvs.py:59-61, 111-113).  The sampling grid carries no gradient (models/module.py:77 builds it under
 * torch.no_grad), the view weights of the iteration branch are detached (models/itermvs.py:295); so the gradient flows to
 * the source features (scatter-add of the four taps, fp32 hardware atomics) and to the reference features (gather; the
 * warped values are recomputed, no [B,C,N,H,W] volume is ever stored).
 *
 * itermvs_corr_iter_backward: `p` = the forward's parameter block (its `out` pointers are ignored);
 *   grad_out[l]   [B,N_l,8,H,W]  dL/d out_l
 *   grad_src[l]   host array of S device pointers: dL/d src_l[s], addressed with the strides of p->src[l]
 *                 (channels-last), ZERO-FILLED by the caller, accumulated into;
 *   grad_ref_q    [B,H,W,C1+C2+C3] dL/d ref_q, written completely.
 * itermvs_corr_init_backward: `p` = the forward's parameter block (p->ref must be channels-last here, N <= 32);
 *   grad_out      [B,S,N,8,H,W]  dL/d out;   grad_src: S device pointers as above (zero-filled);
 *   grad_ref      dL/d ref, addressed with the strides of p->ref: ZERO-FILLED by the caller, accumulated into (several
 *                 workgroups per pixel: one per view and chunk of 8 hypotheses).
 * ------------------------------------------------------------------------------------------ */
int itermvs_corr_iter_backward(const itermvs_corr_iter_params* p, const float* const grad_out[3],
                               float* const* const grad_src[3], float* grad_ref_q, void* stream);
int itermvs_corr_init_backward(const itermvs_corr_init_params* p, const float* grad_out, float* const* grad_src,
                               float* grad_ref, void* stream);

/* itermvs_view_aggregate -- models/itermvs.py:59-69
 *   out[b,n,g,p] = sum_s corr[b,s,n,g,p] * w[b,s,p] / (1e-5 + sum_s w[b,s,p])
 * corr [B,S,N,8,P], w [B,S,P] (PixelViewWeight output at 1/8 res), out [B,N,8,P].  8 * B * N * P <= 2^31 - 1. */
int itermvs_view_aggregate(const float* corr, const float* w, int32_t S, int32_t B, int32_t N,
                           int32_t P, float* out, void* stream);
/* itermvs_view_aggregate_up -- the same, and in the SAME launch (extra blocks: two independent pieces of work that only
 * read w) the x2 bilinear up-sampling of the view weights the iterations use (models/itermvs.py:56-57,71):
 *   w [B,S,H3,W3] -> w_up [B,S,2*H3,2*W3], or, with w_up_interleaved != 0, the same values stored [B,2*H3,2*W3,S] (the
 *   layout itermvs_corr_iter reads fastest: view_w_ss = 1, view_w_sp = S).
 *   corr_layout: 0 = corr [B,S,N,8,P]; 1 = groups last [B,S,N,P,8] (itermvs_corr_init's out_layout 1; 16-byte aligned).
 *   8 * B * N * H3 * W3 <= 2^31 - 1, 4 * B * S * H3 * W3 <= 2^32 - 256, and the two pieces together at most 2^24 - 1 blocks of 256. */
int itermvs_view_aggregate_up(const float* corr, int32_t corr_layout, const float* w, int32_t S, int32_t B, int32_t N, int32_t H3,
                              int32_t W3, float* out, float* w_up, int32_t w_up_interleaved, void* stream);

/* itermvs_softmax_max -- models/itermvs.py:347-348 (PixelViewWeight tail)
 *   out[m,p] = max_n softmax_n(x[m,n,p]);  x [M,N,P] contiguous, out [M,P].  M * P <= 2^32 - 64 (N <= 32), 2^32 - 256 (N > 32). */
int itermvs_softmax_max(const float* x, int32_t M, int32_t N, int32_t P, float* out, void* stream);

/* itermvs_pvw_tail -- models/itermvs.py:343-348 (PixelViewWeight after its 3x3 layer), fused:
 *   out[m,p] = max_n softmax_n( sum_c w[c] * x[m*N+n, c, p] + bias )
 * x [M*N, C, P] planes (C = 16, N <= 32), w [C], bias [1] or NULL, out [M,P].  P <= 2^29 - 64, M <= 65535 (grid.y). */
int itermvs_pvw_tail(const float* x, const float* w, const float* bias, int32_t M, int32_t N, int32_t C,
                     int32_t P, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_prob_regress -- models/itermvs.py:171-190 and :201-219
 *   p = softmax(logits over 256 bins); k* = first argmax p; window k*-4..k*+4 clamped to
 *   [0,255] (duplicates kept); nd = (sum k p_k / (1e-6 + sum p_k)) / 255
 * logits [B,256,H,W] addressed with element strides (sb, sc, sp) where p = y*W+x must be
 * linear (sp = stride between neighbouring pixels).  Outputs (each may be NULL):
 *   nd_out0 / nd_out1: two destinations for the normalised depth, written at
 *     nd_outX[b*nd_sbX + p] (lets the GRU input buffers be filled in place);
 *   prob [B,256,P] contiguous (training / API parity);  best [B,P] int64 arg-max index.
 * P <= 2^29 - 32, B <= 65535 (grid.y).
 * ------------------------------------------------------------------------------------------ */
int itermvs_prob_regress(const float* logits, int64_t sb, int64_t sc, int64_t sp, int32_t B,
                         int32_t P, float* nd_out0, int64_t nd_sb0, float* nd_out1,
                         int64_t nd_sb1, float* prob, int64_t* best, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_head_regress -- the two 1x1 layers of the depth head fused with itermvs_prob_regress
 * (models/itermvs.py:121-126 depth_head[2:5], then :171-190 / :201-219):
 *   y = relu(W1 x); logits = W2 y + b2; nd = window regression of softmax(logits)
 * x [B,32,P] planes (batch stride x_sb) is the output of the head's first (3x3, dilated) layer.
 * Packed weights (fp32):  w1_packed [4][2][4][16][4] with element (mb,u,q,i,s) = W1[mb*16+i][u*16+q*4+s],
 *                         w2_packed [16][4][4][16][4] with element (mb,m,q,i,r) = W2[mb*16+i][m*16+q*4+r];
 * bias2 [256].  Outputs as itermvs_prob_regress (nd_out0 / nd_out1 / best may be NULL); the 256-bin
 * logits are never written to memory.
 * ------------------------------------------------------------------------------------------ */
int itermvs_head_regress(const float* x, int64_t x_sb, int32_t B, int32_t P, const float* w1_packed,
                         const float* w2_packed, const float* bias2, float* nd_out0, int64_t nd_sb0,
                         float* nd_out1, int64_t nd_sb1, int64_t* best, void* stream);

/* itermvs_head_fused -- the whole depth head in one launch: its first layer (3x3, dilation 2, 32 -> 32, ReLU; weights in
 * itermvs_conv2d's weight_format 2 = [9][2][4][32][4]) evaluated from an LDS tile of `hidden` [B,32,H,W] (planes, batch
 * stride hidden_sb) and chained in registers into itermvs_head_regress (models/itermvs.py:121-126, 171-190, 201-219).
 * w2_format: 0 = w2_packed is itermvs_head_regress's fp32 operand layout (exact fp32 matrix instruction);
 *            3 = the 64 -> 256 layer in the bf16x3 form of itermvs_conv2d's weight_format 3 (both operands split exactly into three
 *                bf16 terms, the six largest cross products, fp32 accumulation): w2_packed = bf16 [16][2][3][64][8] whose element
 *                (ob, g, p, lane = 16 q + i, j) is term p of W2[ob*16 + i][(2g + j/4)*16 + 4q + j%4]
 *                (itermvs_amd.ops.pack_head_w2_split3).  w2_packed 16-byte aligned in both forms.
 * w0_format: 0 = w0_tile is the fp32 tile format above; 3 (only together with w2_format 3) = the dilated 3x3 layer in bf16x3 as well:
 *                w0_tile = bf16 [block 2][tap 9][term 3][lane 64][8] whose element (mb, tap, p, 16 q + i, j) is term p of
 *                W0[16 mb + i][(j/4)*16 + 4 q + j%4][tap] (itermvs_amd.ops.pack_head_w0_split3); 16-byte aligned.
 *                itermvs_head_fused_conf takes the fp32 3x3 weights only. */
int itermvs_head_fused(const float* hidden, int64_t hidden_sb, int32_t B, int32_t H, int32_t W,
                       const void* w0_tile, int32_t w0_format, const float* w1_packed, const void* w2_packed, int32_t w2_format,
                       const float* bias2, float* nd_out0, int64_t nd_sb0, float* nd_out1, int64_t nd_sb1, int64_t* best, void* stream);
/* itermvs_head_fused_conf -- itermvs_head_fused and, in the SAME launch on the same staged tile of `hidden`, the confidence
 * head (models/itermvs.py:147-151 with the sigmoid of :198, run on the last GRU iteration :197-199): wc_tile = its dilated
 * 3x3 layer 32 -> 32 in weight_format 2 ([9][2][4][32][4], 16-byte aligned), conf_dot = the 32 weights of its 1x1 layer + bias,
 * conf [B,1,H,W] planes at batch stride conf_sb receives sigmoid(conv1x1(relu(conv3x3(hidden)))). */
int itermvs_head_fused_conf(const float* hidden, int64_t hidden_sb, int32_t B, int32_t H, int32_t W,
                            const float* w0_tile, const float* w1_packed, const void* w2_packed, int32_t w2_format, const float* bias2,
                            float* nd_out0, int64_t nd_sb0, float* nd_out1, int64_t nd_sb1, int64_t* best,
                            const float* wc_tile, const float* conf_dot, float* conf, int64_t conf_sb, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_conv3x3_conv1x1 -- conv3x3 (pad 1) 32 -> 64 + ReLU followed by conv1x1 64 -> NO (+ bias1) in one launch, the
 * 64-channel tensor never stored: IterMVS.upsample (models/itermvs.py:243-247, applied at :262-263; NO = 144, no bias) and
 * Update.hidden_init_head (models/itermvs.py:153-157, applied at :159-160; NO = 32, bias).
 *   x [B,32,H,W] planes (batch stride x_sb); w0_tile = the 3x3 weight in itermvs_conv2d's weight_format 2 = [9][2][4][64][4];
 *   w1_packed [NOB][4][4][16][4] (NOB = ceil(NO/16), zero padded) with element (ob,m,q,i,r) = W1[ob*16+i][m*16+q*4+r];
 *   bias1 [NOB*16] or NULL; out [B,NO,H,W] planes (batch stride out_sb).  All weight pointers 16-byte aligned; NO <= 192.
 *   weight_format 0: the fp32 layouts above (exact fp32 matrix instruction).  weight_format 3: both layers in the bf16x3 form of
 *   itermvs_conv2d's weight_format 3 (operands split exactly into three bf16 terms, six cross products, fp32 accumulation):
 *   w0_tile = bf16 [block 4][tap 9][term 3][lane 64][8] with element (w, tap, p, 16 q + i, j) = term p of
 *   W0[16 w + i][(j/4)*16 + 4 q + j%4][tap]; w1_packed = bf16 [NOB][k group 2][term 3][lane 64][8] with element (ob, g, p, 16 q + i, j) =
 *   term p of W1[ob*16 + i][(2g + j/4)*16 + 4 q + j%4] (itermvs_amd.ops.pack_conv3x3_conv1x1_split3).
 * ------------------------------------------------------------------------------------------ */
int itermvs_conv3x3_conv1x1(const float* x, int64_t x_sb, int32_t B, int32_t H, int32_t W, const void* w0_tile,
                            const void* w1_packed, int32_t weight_format, const float* bias1, int32_t NO, float* out, int64_t out_sb,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_res_chain16 -- the three 3x3 16 -> 16 convolutions that follow the stem in FeatureNet's half-resolution stage
 * (models/net.py:13,40 `layer1` = two ResidualBlocks, models/module.py:33-50; BatchNorm folded) in ONE launch:
 *     a = relu(conv(y1; W0) + b0 + shortcut)     layer1[0].conv2 + layer1[0].downsample's result
 *     b = relu(conv(a;  W1) + b1)                layer1[1].conv1
 *     out = relu(conv(b; W2) + b2 + a)           layer1[1].conv2 + skip
 * a and b never leave LDS.  Arithmetic: the bf16x3 form of itermvs_conv2d's weight_format 3 (both operands split exactly
 * into three bf16 terms, six cross products on v_mfma_f32_16x16x32_bf16, fp32 accumulation).
 *   y1, shortcut [N,16,H,W] (image strides y1_sn / shortcut_sn, elements): itermvs_stem's two results, in_layout = the
 *   out_layout they were written with (0 planes, 1 channel quads [N,4,H,W,4]: a quarter of the load instructions);
 *   weights[3]: each layer's weight in weight_format 3 = bf16 [9][1][3][16][16] (itermvs_amd.ops.MfmaWeight(...).tile3), 16-byte
 *   aligned; bias[3]: 16 floats each (NULL = none); out [N,16,H,W] planes.  H, W <= 4095.
 * ------------------------------------------------------------------------------------------ */
int itermvs_res_chain16(const float* y1, int64_t y1_sn, const float* shortcut, int64_t shortcut_sn, int32_t in_layout, int32_t N,
                        int32_t H, int32_t W, const void* const* weights, const float* const* bias, float* out, int64_t out_sn, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_down_conv -- the stride-2 pair of a FeatureNet residual block (models/net.py:14-15 `layer2`, `layer3`: the first
 * ResidualBlock's conv1 and downsample read the same input, models/module.py:33-50; BatchNorm folded) in ONE launch:
 *     y  = relu(conv3x3_s2(x; W1) + b1)          [N,C,Ho,Wo]
 *     sc =      conv3x3_s2(x; Wd) + bd           [N,C,Ho,Wo]      padding 1, Ho = (H-1)/2 + 1, Wo = (W-1)/2 + 1
 * A workgroup stages and splits each input tile once for all 2C output channels.  Arithmetic: the bf16x3 form of
 * itermvs_conv2d's weight_format 3 (both operands split exactly into three bf16 terms, six cross products on
 * v_mfma_f32_16x16x32_bf16, fp32 accumulation).
 *   x [N,Cin,H,W] planes (image stride x_sn, elements); (Cin, C) = (16, 32) or (32, 48), anything else returns
 *   ITERMVS_ERR_CHANNELS; w_packed: the weight of cat(W1, Wd) [2C,Cin,3,3] in weight_format 3 = bf16 [9][Cin/16][3][2C][16]
 *   (itermvs_amd.ops.MfmaWeight(...).tile3), 16-byte aligned; bias: 2C floats (b1, bd) or NULL; y, sc planes with image
 *   strides y_sn, sc_sn.  H, W <= 4095, Cin H W <= 2^28.
 * ------------------------------------------------------------------------------------------ */
int itermvs_down_conv(const float* x, int64_t x_sn, int32_t N, int32_t Cin, int32_t H, int32_t W, const void* w_packed,
                      const float* bias, int32_t C, float* y, int64_t y_sn, float* sc, int64_t sc_sn, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_lateral_conv3x3 -- one level of FeatureNet's top-down path in ONE launch (models/net.py:48-50; test mode :62-63):
 *     intra = F.interpolate(coarse, scale_factor=2, mode="bilinear") + inner(fine)       1x1 layer Cf -> 48, bias
 *     out   = output(intra)                                                               3x3 layer 48 -> Cout, bias, padding 1
 * `intra` ([N,48,H,W]; 78 MB at level 1 of cfg 1) never reaches memory: only the output convolution reads it (net.py:50).
 * Arithmetic: the 1x1 layer on the exact fp32 matrix instruction, the up-sampling operation for operation that of
 * itermvs_bilinear_up (align_corners=False), the 3x3 layer in the bf16x3 form of itermvs_conv2d's weight_format 3.
 *   fine [N,Cf,H,W] planes (image stride fine_sn), coarse [N,48,H/2,W/2] planes (coarse_sn); H, W even; Cf = 16, Cout = 16
 *   (ITERMVS_ERR_CHANNELS otherwise: the level-1 layer pair of the path);
 *   w_lat: the 1x1 weight in weight_format 1 = fp32 [Cf][48] (itermvs_amd.ops.MfmaWeight(...).data), b_lat [48] or NULL;
 *   w_out: the 3x3 weight in weight_format 3 = bf16 [9][3][3][16][16] (MfmaWeight(...).tile3), 16-byte aligned; b_out [Cout] or NULL;
 *   out: out_layout 0 = fp32 planes [N,Cout,H,W]; 1 / 2 / 3 = channels-last [N,H,W,Cout] in fp32 / fp16 / bf16 storage (what the
 *   correlation kernels gather from; out_sn in ELEMENTS of the storage type); out2: optional dense fp32 planar copy or NULL.
 * ------------------------------------------------------------------------------------------ */
int itermvs_lateral_conv3x3(const float* fine, int64_t fine_sn, int32_t Cf, const float* coarse, int64_t coarse_sn, int32_t N,
                            int32_t H, int32_t W, const float* w_lat, const float* b_lat, const void* w_out, const float* b_out,
                            int32_t Cout, void* out, int64_t out_sn, int32_t out_layout, float* out2, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_gru_conv -- the dilated 3x3 convolutions of the ConvGRU with their gate math, as cooperative bf16x3 kernels
 * (models/module.py:53-66; the GRU of models/itermvs.py:131-137: 32 hidden + 1 + 10 input channels, dilation 2, padding 2).
 *   mode 0: x = [h | inputs] [B,43,H,W];  z = sigmoid(convz(x)) -> out [B,32,H,W];  r = sigmoid(convr(x)), r * h -> out2
 *           (module.py:61-63).  w_packed / bias: the two layers stacked along the output channels (64).
 *   mode 1: x = [r*h | inputs];  q = tanh(convq(x));  h' = (1 - z) h + z q -> out (and out2 when not NULL)  (module.py:64-65).
 *           h may alias out (every element is read before it is written, by the same thread).
 * x, h, z, out, out2: fp32 channel planes of H*W elements (row stride W), batch strides *_sb in elements.
 * w_packed (16-byte aligned): bf16 [output block of 16][tap 9][operand 6][lane 64][8]; with lane = 16 q + i and (h, m, l) the exact
 * three-term bf16 split of W[16 ob + i][c][tap]:  operands 0..2 = h, m, l of channel c = (j / 4) * 16 + 4 q + j % 4;  operands
 * 3..5 of channel c = 32 + 8 (q % 2) + j (zero from 43 on) = h, m and (q < 2 ? l : h).
 * Arithmetic: fp32 accumulation of the six largest cross products (a few 1e-7 of the fp32 form's range; tests/test_kernels_gpu.py).
 * Replaces, in the inference step, two itermvs_conv2d launches per GRU iteration.
 * ------------------------------------------------------------------------------------------ */
int itermvs_gru_conv(const float* x, int64_t x_sb, int32_t B, int32_t H, int32_t W, int32_t mode, const void* w_packed,
                     const float* bias, const float* h, int64_t h_sb, const float* z, int64_t z_sb, float* out, int64_t out_sb,
                     float* out2, int64_t out2_sb, void* stream);



/* ------------------------------------------------------------------------------------------
 * ConvGRU gates -- models/module.py:59-66 (element-wise form for the traced / training path; in the inference
 * engine the gate math rides in the epilogue of the dilated 3x3 convolutions, itermvs_conv2d act 4/5)
 * itermvs_gru_rh :  rh[b,c,p] = sigmoid(zr[b,32+c,p]) * h[b,c,p]           (r * h, :63-64)
 * itermvs_gru_out:  h[b,c,p]  = (1-z) * h + z * tanh(q),  z = sigmoid(zr[b,c,p])   (:62,64,65)
 * zr = [B,2*hid,P] (z pre-activations then r pre-activations), q = [B,hid,P];
 * h / rh are addressed as base + b*sb + c*P + p so they can live inside the [B,43,P]
 * concatenated GRU input buffers.  itermvs_gru_out updates h in place and, when h_copy != NULL,
 * also stores the new state contiguously at h_copy[B,hid,P] (input of the depth / confidence head convolutions).
 * B * hid * P <= 2^32 - 256.
 * ------------------------------------------------------------------------------------------ */
int itermvs_gru_rh(const float* zr, const float* h, int64_t h_sb, float* rh, int64_t rh_sb,
                   int32_t B, int32_t hid, int32_t P, void* stream);
int itermvs_gru_out(const float* zr, const float* q, float* h, int64_t h_sb, float* h_copy,
                    int32_t B, int32_t hid, int32_t P, void* stream);

/* itermvs_pack_scores -- models/itermvs.py:122-124,193: concatenates the three CorrNet outputs
 * ([B,N_l,P] each) into channels [ch0, ch0+N0+N1+N2) of up to two [B,Ctot,P] buffers.  B * (N0+N1+N2) * P <= 2^31 - 1. */
int itermvs_pack_scores(const float* s0, const float* s1, const float* s2, const int32_t N[3],
                        int32_t B, int32_t P, float* dst0, float* dst1, int64_t dst_sb,
                        int32_t ch0, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_convex_upsample -- models/itermvs.py:262-264 (softmax over the 9 taps) +
 * models/module.py:127-140 (upsample) + models/module.py:148-152 (depth_unnormalization)
 *   logits [B,144,H,W] (element strides sb,sc,sy,sx; channel = k*16 + i*4 + j)
 *   nd     [B,1,H,W] at nd + b*nd_sb + y*W + x
 *   depth  [B,1,4H,4W] contiguous = 1/(inv_max + up*(inv_min-inv_max));
 *   when `norm_out` != NULL the un-normalised convex combination is also stored there.
 *   4 * B * H * W <= 2^31 - 1.
 * ------------------------------------------------------------------------------------------ */
int itermvs_convex_upsample(const float* logits, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                            const float* nd, int64_t nd_sb, const float* inv_depth_min,
                            const float* inv_depth_max, int32_t B, int32_t H, int32_t W,
                            float* depth, float* norm_out, void* stream);
/* itermvs_final_upsample -- itermvs_convex_upsample (depth, models/itermvs.py:321-322) and, in the SAME launch, the x4 bilinear
 * up-sampling of the confidence (models/itermvs.py:323-324): conf [M,H,W] -> conf_up [M,4H,4W].
 * 4 * B * H * W <= 2^31 - 1, 16 * M * H * W <= 2^32 - 256, and the two pieces together at most 2^24 - 1 blocks of 256. */
int itermvs_final_upsample(const float* logits, int64_t sb, int64_t sc, int64_t sy, int64_t sx, const float* nd, int64_t nd_sb,
                           const float* inv_depth_min, const float* inv_depth_max, int32_t B, int32_t H, int32_t W, float* depth,
                           const float* conf, int32_t M, float* conf_up, void* stream);

/* itermvs_bilinear_up -- F.interpolate(x, scale_factor=s, mode='bilinear') for integer s
 * (models/itermvs.py:56,161,323): x [M,H,W] -> out [M,s*H,s*W]; `act`: 0 none, 1 tanh
 * (hidden_init, itermvs.py:162).  M * H * W * s^2 <= 2^32 - 256 (itermvs_bilinear_up2: B * C * H * W * s^2). */
int itermvs_bilinear_up(const float* x, int32_t M, int32_t H, int32_t W, int32_t scale,
                        int32_t act, float* out, void* stream);
/* same for x [B,C,H,W] with up to two destinations given as [C,sH,sW] planes at batch strides out_sb / out2_sb
 * (elements): lets the initial hidden state (itermvs.py:161-163) land in `hidden` and in channels 0..31 of the
 * GRU input buffer in one launch.  out2 may be NULL. */
int itermvs_bilinear_up2(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, int32_t scale, int32_t act,
                         float* out, int64_t out_sb, float* out2, int64_t out2_sb, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_conv2d -- the small-channel 2-D convolutions of the path, with fused epilogues:
 *   nn.Conv2d / ConvBnReLU (BN folded) / ConvReLU      models/module.py:6-30
 *   ResidualBlock's relu(x + y)                        models/module.py:33-50
 *   nn.ConvTranspose2d(3, stride 2, pad 1, out_pad 1)  models/itermvs.py:359-363 (CorrNet)
 *   ConvGRU gates                                      models/module.py:59-66
 * fp32, contiguous [C,H,W] planes; `in_sn` / `out_sn` / ... are BATCH strides in elements, so
 * inputs and outputs may be channel slices of wider buffers.  `weight` is PACKED:
 *   weight_format 0: [Cin][k][k][Cout] (conv weight.permute(1,2,3,0); transposed-conv
 *     weight.permute(0,2,3,1)) -- VALU kernels, required for `transposed`;
 *   weight_format 1: [k*k][Cin_pad4][Cout_pad16], zero padded -- matrix-core (MFMA f32 16x16x4)
 *     implicit-GEMM kernel (any 1x1 / 3x3 shape);
 *   weight_format 2: [9][chunks][4][Cout_pad16][S] with element (tap, ch, q, co, s) = weight of input
 *     channel ch*4*S + q*S + s (S = 1 / 2 / 4 for Cin <= 4 / <= 8 / larger), zero padded -- the LDS-tiled
 *     persistent matrix-core kernel for 3x3, stride 1|2, dilation 1|2;
 *   weight_format 3: bfloat16 [9][chunks][3][Cout_pad16][16] with element (tap, ch, p, co, c) = term p of the exact
 *     three-term bf16 split (h = w truncated to 8 significant bits, m = (w - h) truncated, l = w - h - m) of the weight of
 *     input channel ch*16 + c, zero padded -- the same LDS-tiled kernel on v_mfma_f32_16x16x32_bf16 for 3x3 layers with
 *     Cin > 8: activations are split the same way when staged, the six largest cross terms are accumulated in fp32
 *     (error ~2^-23 per product: fp32-rounding class, NOT bit-identical to the fp32 forms).  Up to three weight sets
 * per launch: batch items [0,seg_end[0]) use set 0, [seg_end[0],seg_end[1]) set 1, the rest set 2
 * (the three CorrNets of one iteration in one launch).
 * Epilogue `act`: 0 v+add | 1 relu(v+add) | 2 sigmoid | 3 tanh | 4 sigmoid(v)*aux1 (r*h) |
 *                 5 (1-aux2)*aux1 + aux2*tanh(v)  (GRU state update; aux1 = h, aux2 = z) |
 *                 6 sum_co relu(v[co]) * aux1[co] + aux1[Cout]: a following 1x1 convolution to ONE channel folded into the
 *                   epilogue (PixelViewWeight, models/itermvs.py:337-346); Cout = 16 or 32, 3x3, weight_format 2, `out` is the
 *                   single plane [N,1,H,W] (batch stride out_sn), aux1 = Cout + 1 floats shared by all batch items
 *                   (aux1_sn = 0) |
 *                 7 sigmoid of 6 (the confidence head, models/itermvs.py:147-151,198).
 * `add_mode` 0: `add` has the output's shape; 1: `add` is [N,Cout,Hout/2,Wout/2] and its x2 bilinear
 *   up-sampling (F.interpolate(scale_factor=2, mode='bilinear'), models/net.py:46,49) is evaluated
 *   in the epilogue (matrix-core formats only, Hout and Wout even).
 * `out_layout` 0: `out` is [Cout,H,W] planes per batch item (batch stride out_sn); 1: `out` is a dense
 *   channels-last [N,H,W,Cout] tensor (the layout the correlation kernels read; act 0, no `add`,
 *   Cout % 4 == 0, matrix-core formats only); 2 / 3: the same in fp16 / bf16 storage (round to nearest even of the
 *   fp32 result; `out` points to 16-bit elements, out_sn counts them).
 * `out2` (optional) receives a second, contiguous [N,Cout,H,W] copy of the result.
 * `split_cout` > 0 (matrix-core formats, multiple of 16): output channels [split_cout, Cout) form a SECOND
 *   result with its own activation `act_b` and destination `out_b` (planes, batch stride out_b_sn, channel
 *   index rebased to 0); channels [0, split_cout) go to `out` with `act`.  One launch then evaluates two
 *   convolutions of the same input -- the ConvGRU update and reset gates (models/module.py:61-63).
 * ------------------------------------------------------------------------------------------ */
typedef struct itermvs_conv_params {
    const float* in;
    float* out;
    float* out2;
    const float* add;
    const float* aux1;
    const float* aux2;
    int64_t in_sn, out_sn, add_sn, aux1_sn, aux2_sn;
    const float* weight[3];
    const float* bias[3];                      /* [Cout] or NULL */
    int32_t seg_end[3];
    int32_t n_seg;
    int32_t N, Cin, Hin, Win, Cout;
    int32_t ksize, stride, pad, dilation;      /* ksize 1 or 3 */
    int32_t transposed;                        /* 1: ConvTranspose2d(3, stride 2, pad 1, output_padding 1) */
    int32_t act;
    int32_t weight_format;
    int32_t add_mode;
    int32_t out_layout;
    int32_t split_cout;
    int32_t act_b;
    int32_t in_layout;                         /* 0 = `in` [N,Cin,Hin,Win] planes; 1 = channels last [N,Hin,Win,8] -- only the 3x3 layers with
                                                * exactly 8 input channels in weight_format 3 (stride 1, no dilation: PixelViewWeight's layer
                                                * reading itermvs_corr_init's out_layout 1); `in` 16-byte aligned, in_sn a multiple of 4 */
    float* out_b;
    int64_t out_b_sn;
} itermvs_conv_params;

int itermvs_conv2d(const itermvs_conv_params* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_conv2d_plan -- diagnostic (ABI 19): WHICH kernel itermvs_conv2d runs for `p`.  Runs exactly the validation and the
 * kernel choice of itermvs_conv2d and returns: same status for every rejected block, ITERMVS_OK and `*plan` otherwise.  It
 * never reads through the data pointers (only whether they are set) and makes no device call, so it works on host memory and
 * without a GPU.  Fields that do not apply to the back end are 0.
 * ------------------------------------------------------------------------------------------ */
typedef enum itermvs_conv_backend {
    ITERMVS_CONV_DIRECT = 0,        /* conv_direct_kernel<CT, KS>                          weight_format 0 */
    ITERMVS_CONV_MFMA = 1,          /* conv_mfma_kernel<MB, NB, KS>                        weight_format 1 */
    ITERMVS_CONV_MFMA_SPLITK = 2,   /* conv_mfma_splitk_kernel<MB, KS> */
    ITERMVS_CONV_LATERAL_UP2 = 3,   /* lateral_up2_kernel<MB> */
    ITERMVS_CONV_TILE = 4,          /* conv_tile_kernel<MB, S, STRIDE, DIL, TH, TWT, CPS>  weight_format 2 */
    ITERMVS_CONV_DECONV = 5,        /* deconv_tile_kernel<MB, S, TH, NCH> */
    ITERMVS_CONV_TILE3 = 6,         /* conv_tile3_kernel<MB, STRIDE, DIL, TH, TWT, CPS>    weight_format 3 */
    ITERMVS_CONV_TILE3_PAIR = 7     /* conv_tile3_kernel<MB, 1, 1, 8, 2, 1, 1, INCL> */
} itermvs_conv_backend;

typedef struct itermvs_conv_plan {
    int32_t backend;                                   /* itermvs_conv_backend */
    int32_t MB, NB, CT, KS, S, STRIDE, DIL, TH, TWT, CPS, NCH, PAIR, INCL;   /* template arguments of the kernel */
    int32_t lds_bytes;                                 /* dynamic LDS of the launch */
    int32_t tiles_x, tiles_y, ncb, nstage, total;      /* tile grid, channel blocks, stages per tile, N * tiles_y * tiles_x */
    int32_t Hout, Wout;
} itermvs_conv_plan;

int itermvs_conv2d_plan(const itermvs_conv_params* p, itermvs_conv_plan* plan);

/* ------------------------------------------------------------------------------------------
 * itermvs_persistent_plan / itermvs_tile_walk_owner -- diagnostics (ABI 20): the grid rule and the tile walks of the persistent
 * kernels (csrc/tile_walk.hpp; DESIGN.md lists which kernel uses which), run on the host.  Neither makes a device call.
 *   itermvs_persistent_plan: the launch of `tiles` tiles (1 .. 2^31 - 1, else ITERMVS_ERR_DIMS) by at most `resident` workgroups:
 *     grid = min(tiles, resident), rounded down to a multiple of 8 from 16 on when `round8`; whether the XCD-banded tile order
 *     applies; for ITERMVS_WALK_RUNS the split of the tile list into runs.  STRIDED_LEAD: `grid` counts the tile workgroups only.
 *   itermvs_tile_walk_owner: runs the kernels' own walk for every workgroup of `plan` (`lead` extra workgroups in front for
 *     ITERMVS_WALK_STRIDED_LEAD, else 0) and writes, per tile, owner[t] = the workgroup that visits it (STRIDED_LEAD: counted from
 *     the first tile workgroup; -1: none) and order[t] = its position in that workgroup's sequence.  Returns the number of
 *     visits to an already visited tile (0 for a correct walk), or a negative status.
 * ------------------------------------------------------------------------------------------ */
typedef enum itermvs_walk_kind {
    ITERMVS_WALK_STRIDED = 0,       /* conv_tile, conv_tile3, res_chain16, lat_conv: tiles w, w + wstep, ... of the list or of an eighth */
    ITERMVS_WALK_RUNS = 1,          /* gru_conv, down_conv: one run of consecutive tiles per workgroup */
    ITERMVS_WALK_PLAIN = 2,         /* stack2, head_coop: tiles b, b + grid, ... */
    ITERMVS_WALK_STRIDED_LEAD = 3   /* stem: STRIDED behind `lead` workgroups that do other work, banded from 8 tile workgroups on */
} itermvs_walk_kind;

typedef struct itermvs_persistent_plan_t {
    int32_t grid, banded, run, run_extra;
} itermvs_persistent_plan_t;

int itermvs_persistent_plan(int64_t tiles, int32_t resident, int32_t round8, int32_t kind, itermvs_persistent_plan_t* out);
int itermvs_tile_walk_owner(const itermvs_persistent_plan_t* plan, int64_t tiles, int32_t kind, int32_t lead, int32_t* owner, int32_t* order);

/* ------------------------------------------------------------------------------------------
 * itermvs_corrnet -- the whole CorrNet (models/itermvs.py:352-381: conv0..conv2, the two transposed convolutions with
 * their skip additions, conv5 + bias) in ONE launch, every intermediate in LDS (32 x 32 output tiles, halos recomputed).
 *   x [M,8,H,W] planes (batch stride x_sn), H and W multiples of 4;  out / out2 (optional) [M,1,H,W] at batch strides
 *   out_sn / out2_sn (the GRU input buffers take the scores in place);
 *   weights: host array of n_seg (1..3) device pointers to PACKED weight sets, batch items [0,seg_end[0]) use set 0,
 *   [seg_end[0],seg_end[1]) set 1, the rest set 2 (the three CorrNets of one GRU iteration in one launch).
 *   Packed set (fp32, 14288 floats, 16-byte aligned): the five matrix-core layers in operand order
 *   [tap = ky*3+kx][k-step = ci/4][q = ci%4][co, zero padded] -- conv0 in its two-rows-per-tile form ([window row 4][kx 3]
 *   [k-step][q][16]: columns 0..7 = channel co with tap row = window row, columns 8..15 = channel co - 8 with tap row =
 *   window row - 1, zero where that is outside 0..2) | conv1 (16) | conv2 (32) | conv3, transposed (16) | conv4, transposed
 *   (16) -- then conv5 as [ci 8][tap 9], the bias, 7 pad (itermvs_amd.ops.pack_corrnet_weights).
 * ------------------------------------------------------------------------------------------ */
int itermvs_corrnet(const float* x, int64_t x_sn, const float* const* weights, const int32_t* seg_end, int32_t n_seg,
                    int32_t M, int32_t H, int32_t W, float* out, int64_t out_sn, float* out2, int64_t out2_sn, void* stream);
/* itermvs_corrnet_bf16x3 -- the same launch with conv0, conv2 and the two transposed convolutions on v_mfma_f32_16x16x32_bf16:
 * both operands split EXACTLY into three bf16 terms, the six largest cross products accumulated in fp32 (error of the size of one
 * fp32 rounding per product, like itermvs_conv2d's weight_format 3); conv1 stays on the fp32 instruction (its input is kept in fp32
 * for the skip connection and the last layer).  Packed set: 23120 floats = conv0 as bf16 A operands [18 MFMAs][64 lanes][8 bf16]
 * (4608 floats: MFMA 2v / 2v+1 = terms h / m of the window-position pair v, 12 + v = [l l | h h]; lane (q, m): window position
 * 2v + (q & 1), output row-channel m as in the fp32 form) | conv1 as in itermvs_corrnet (1152 floats) | conv2, conv3, conv4 in
 * weight_format 3 = bf16 [tap 9][chunk ci/16][term h, m, l][row co][16 ci] with 32 / 16 / 16 rows (6912 + 6912 + 3456 floats; a
 * transposed convolution as the convolution weight [co][ci][ky][kx] = w[ci][co][ky][kx]) | conv5 [ci 8][tap 9], the bias, 7 pad
 * (itermvs_amd.ops.pack_corrnet_weights(split3=True)). */
int itermvs_corrnet_bf16x3(const float* x, int64_t x_sn, const float* const* weights, const int32_t* seg_end, int32_t n_seg,
                           int32_t M, int32_t H, int32_t W, float* out, int64_t out_sn, float* out2, int64_t out2_sn, void* stream);


/* ------------------------------------------------------------------------------------------
 * itermvs_stem -- the first two layers of FeatureNet in ONE launch (models/net.py:13-14,39-40; models/module.py:33-50):
 * FeatureNet.conv1 (ConvBnReLU 3 -> 8) and, from its result without a round trip through HBM, layer1[0].conv1
 * (ConvBnReLU 8 -> 16, stride 2) and layer1[0].downsample (ConvBn 8 -> 16, stride 2).  BatchNorm folded by the caller.
 *   x [M,3,H,W] planes (batch stride x_sn);  y = relu(conv1 branch), sc = downsample branch: [M,16,H2,W2] planes at batch
 *   stride out_sn, H2 = (H-1)/2+1;
 *   w0: 224 floats = conv1 weight as [ci][ky][kx][co 8] then its 8 biases;
 *   w1: 2336 floats = the two stride-2 layers' weights, output channels concatenated (conv1 branch first), in matrix-core
 *   operand order [tap = ky*3+kx][k-step = ci/4][q = ci%4][co 32], then the 32 biases (itermvs_amd.ops.pack_stem_weights).
 *   out_layout: 0 = planes [M,16,H2,W2]; 1 = channel quads [M,4,H2,W2,4] (channel 4*cq + c of pixel p at ((cq*H2*W2 + p)*4 + c):
 *   the layout itermvs_res_chain16 fetches with 16-byte loads; y, sc 16-byte aligned, out_sn a multiple of 4).
 * ------------------------------------------------------------------------------------------ */
int itermvs_stem(const float* x, int64_t x_sn, int32_t M, int32_t H, int32_t W, const float* w0, const float* w1,
                 float* y, float* sc, int64_t out_sn, int32_t out_layout, void* stream);
/* itermvs_stem_compose -- itermvs_stem and, in the SAME launch (its first workgroup), itermvs_compose_proj with its arguments
 * (mats .. inv_max; Bd = batch size of the depth range; module.py:77-90, itermvs.py:267-268): the composition depends on the
 * cameras only, so its ~10 us fp64 chain hides behind the first, longest launch of FeatureNet. */
int itermvs_stem_compose(const float* x, int64_t x_sn, int32_t M, int32_t H, int32_t W, const float* w0, const float* w1,
                         float* y, float* sc, int64_t out_sn, int32_t out_layout, const float* mats, int32_t n_sets, int32_t V, float* proj_out,
                         int32_t* nan_flag, const float* depth_min, const float* depth_max, int32_t Bd, float* inv_min,
                         float* inv_max, void* stream);



/* ------------------------------------------------------------------------------------------
 * itermvs_fuse_depth -- the filter that follows the depth-inference path:
 *   reproject_with_depth (eval.py:154-194), check_geometric_consistency (eval.py:197-212) and the per-reference
 *   arithmetic of filter_depth (eval.py:238-269) for ONE reference view against its S source views, one pass.
 * depth_ref / conf_ref [H,W] fp32; depth_src: HOST array of S device pointers to [H,W] fp32 depth maps;
 * mats: device [S][60] fp32 = per pair  inv(K_ref)(9) | (E_src inv(E_ref)) rows 0..2 (12) | K_src(9) | inv(K_src)(9) |
 *   (E_ref inv(E_src)) rows 0..2 (12) | K_ref(9), inverted / composed on the host in float32 like eval.py does.
 * Outputs: depth_avg [H,W] fp64 = (sum of consistent reprojected depths + depth_ref) / (count + 1); optional uint8
 *   masks photo (conf > photo_thres), geo (count >= geo_mask_thres), final (both); optional int32 count.
 * ------------------------------------------------------------------------------------------ */
int itermvs_fuse_depth(const float* depth_ref, const float* conf_ref, const float* const* depth_src,
                       const float* mats, int32_t S, int32_t H, int32_t W, double geo_pixel_thres,
                       float geo_depth_thres, float photo_thres, int32_t geo_mask_thres, double* depth_avg,
                       uint8_t* photo_mask, uint8_t* geo_mask, uint8_t* final_mask, int32_t* geo_sum,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_fuse_depth_claim -- itermvs_fuse_depth with a claim step behind it, so that a surface point seen by N views is
 *   emitted once per scan (eval.py --fuse_dedupe).  The caller keeps one map claimed[v], uint8 [H,W], per view of the scan, all
 *   zero at the start of the scan, and fuses the reference views in pair.txt order on one stream.  For reference view r, pixel p:
 *   1. depth_avg, photo, geo, the count and per source s the consistency decision ok_s are those of itermvs_fuse_depth, bit for
 *      bit (eval.py:238-269; same per-pixel code).
 *   2. final[p] = photo && geo && claimed_ref[p] == 0.  photo_mask and geo_mask are unchanged; final_mask is the emit mask.
 *   3. If final[p], for every source s with ok_s: with (xs, ys) the fp32 source coordinates of p and smp the fp32 bilinear
 *      sample of depth_src[s] there (both as in step 1), qx = rintf(xs), qy = rintf(ys); if 0 <= qx <= W-1 and 0 <= qy <= H-1
 *      (compared in fp32, so NaN and inf fail) and fabsf(depth_src[s][qy*W+qx] - smp) / smp < geo_depth_thres in fp32 (false
 *      or NaN: no claim), then claimed_src[s][qy*W+qx] = 1.  The second condition keeps a nearest pixel that lies across a depth
 *      edge from being suppressed by a point it does not represent.
 *   Step 3 has no counterpart in the reference (it is the used-pixel marking of Gipuma's fusibile); steps 1 and 2 with all maps
 *   zero are eval.py:238-269.  The vertices are what itermvs_fuse_points makes of depth_avg and this final_mask.
 * claimed_ref: device [H,W] uint8, read only; NULL = all zero.  claimed_src: HOST array of S device pointers to [H,W] uint8
 *   maps, only ever written, with plain byte stores of the constant 1 (no atomics, no order between workgroups: the result does
 *   not depend on scheduling); NULL = step 3 is skipped.  Every other argument as in itermvs_fuse_depth, same launch shape.
 * Validation before the launch: the checks of itermvs_fuse_depth, then ITERMVS_ERR_NULL for a NULL entry of claimed_src and
 *   ITERMVS_ERR_DIMS when a claimed_src[s] == claimed_ref (the launch would race with itself; r is never its own source).
 * ------------------------------------------------------------------------------------------ */
int itermvs_fuse_depth_claim(const float* depth_ref, const float* conf_ref, const float* const* depth_src,
                             const float* mats, int32_t S, int32_t H, int32_t W, double geo_pixel_thres,
                             float geo_depth_thres, float photo_thres, int32_t geo_mask_thres, double* depth_avg,
                             uint8_t* photo_mask, uint8_t* geo_mask, uint8_t* final_mask, int32_t* geo_sum,
                             const uint8_t* claimed_ref, uint8_t* const* claimed_src, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_fuse_depth_dynamic -- itermvs_fuse_depth_claim with dynamic geometric consistency in place of the count against
 *   geo_mask_thres (eval.py --geo_consistency dynamic): few source views that agree tightly are accepted, and so are many that
 *   agree loosely, with no per-scene number (the dynamic consistency checking of D2HC-RMVSNet).  For one reference pixel p:
 *   Per source s, unchanged from itermvs_fuse_depth (same expressions, same bits): dist_s fp64, the pixel distance of the
 *     reprojection (eval.py:203); rel_s fp32, its relative depth difference (eval.py:205-206); ok_s = dist_s < geo_pixel_thres
 *     && rel_s < geo_depth_thres, the base decision.
 *   Levels: s passes level n iff dist_s < (double)n * dyn_pixel_step && rel_s < (float)n * dyn_depth_step -- each product
 *     rounded once, the comparisons strict, NaN fails.  c_n = number of sources that pass level n.
 *     level = the smallest n in [n_min, min(n_max, S)] with c_n >= n, or 0 if there is none.
 *   Masks: geo = level != 0; photo = conf > photo_thres; final = photo && geo && claimed_ref[p] == 0.
 *   depth_avg, the count geo_sum and the claim step (step 3 of itermvs_fuse_depth_claim) are bit for bit those of
 *     itermvs_fuse_depth / itermvs_fuse_depth_claim on the same inputs: the average is taken over the sources with ok_s and the
 *     claims are made for the sources with ok_s.  There is no geo_mask_thres.
 *   The reference has no counterpart of the level rule (like step 3 of itermvs_fuse_depth_claim).  The driver's defaults,
 *     dyn_pixel_step 0.25, dyn_depth_step (float)(1.0 / 1300), levels 2..10, are written from memory of the published code
 *     and are UNVERIFIED.
 * claimed_ref, claimed_src: as in itermvs_fuse_depth_claim, either may be NULL; both NULL is the form without the claim maps.
 * geo_level: optional device [H,W] uint8, receives level.  No LDS, no atomics, one pass; the launch shape of itermvs_fuse_depth.
 * Validation before any HIP call: the checks of itermvs_fuse_depth_claim in its order, then ITERMVS_ERR_DIMS unless
 *   dyn_pixel_step and dyn_depth_step are finite and > 0 and 1 <= n_min <= n_max <= ITERMVS_MAX_SRC (n_max > S is allowed).
 * ------------------------------------------------------------------------------------------ */
int itermvs_fuse_depth_dynamic(const float* depth_ref, const float* conf_ref, const float* const* depth_src,
                               const float* mats, int32_t S, int32_t H, int32_t W, double geo_pixel_thres,
                               float geo_depth_thres, float photo_thres, double* depth_avg, uint8_t* photo_mask,
                               uint8_t* geo_mask, uint8_t* final_mask, int32_t* geo_sum, const uint8_t* claimed_ref,
                               uint8_t* const* claimed_src, double dyn_pixel_step, float dyn_depth_step, int32_t n_min,
                               int32_t n_max, uint8_t* geo_level, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_fuse_points -- the tail of filter_depth for ONE reference view (eval.py:287-308): the pixels of `final_mask` are
 *   unprojected (eval.py:287-294), coloured (eval.py:295-296) and appended to `records` as the PLY vertex element of
 *   eval.py:298-308 (x, y, z little-endian float32; red, green, blue uint8: 15 bytes per vertex, unpadded), in row-major pixel
 *   order (y, then x) behind the vertices of the views emitted before -- the order of the reference's boolean indexing.
 *   Three launches on `stream` (count, single-workgroup scan, emit); no workgroup waits on another and nothing is accumulated
 *   with atomics, so the bytes do not depend on scheduling.  Calls for consecutive views may be enqueued back to back: the host
 *   reads nothing between them.
 * depth_avg [H,W] fp64, final_mask / photo_mask / geo_mask [H,W] uint8 as itermvs_fuse_depth wrote them (photo_mask, geo_mask
 *   may be NULL: they are only counted); cam: device [21] fp32 = inv(K_ref) (9) | rows 0..2 of inv(E_ref) (12), inverted on the
 *   host in float32; rgb [H,W,3] uint8, the reference image at the depth maps' size (copied: (u / 255.f * 255) cast back to
 *   uint8 is u for every byte value).
 * Arithmetic: pixel indices as fp64, x*d, y*d, d, then (m0*p0 + m1*p1) + m2*p2 and ((..) + m2*p2) + m3*1.0 in fp64 without
 *   fused multiply-add, one round-to-nearest conversion to fp32; non-finite values pass through.
 * records: `capacity` vertices of 15 bytes, shared by the views of a flush group (may be NULL when capacity is 0);
 * cursor: device uint64, vertices emitted so far: read as this view's first vertex index and advanced by its count ON THE DEVICE;
 * view_counts: device int64 [n_views][4]; row `view` receives {pixels in photo_mask, in geo_mask, in final_mask, first vertex
 *   index} (-1 for a mask that was not given).
 * A vertex whose index is >= capacity is not stored; cursor and view_counts hold the true totals all the same, so the caller
 *   sees the overflow (cursor > capacity) at its next synchronisation.  Nothing outside records[0 : 15 * capacity] is written.
 * workspace: itermvs_fuse_points_workspace_bytes(H, W) bytes of device scratch (per-workgroup counts), reusable by the next
 *   call on the same stream.  ITERMVS_ERR_DIMS: H or W < 1, H * W > 0x7fffff00 (32-bit pixel indices), capacity or view < 0.
 * ------------------------------------------------------------------------------------------ */
int itermvs_fuse_points_workspace_bytes(int32_t H, int32_t W);
int itermvs_fuse_points(const double* depth_avg, const uint8_t* final_mask, const uint8_t* photo_mask,
                        const uint8_t* geo_mask, const float* cam, const uint8_t* rgb, int32_t H, int32_t W,
                        uint8_t* records, int64_t capacity, uint64_t* cursor, int64_t* view_counts, int32_t view,
                        uint32_t* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_fuse_points_normals -- itermvs_fuse_points with an oriented unit normal per vertex (eval.py --ply_normals; no
 *   counterpart in the reference, the vertex layout is COLMAP's fused.ply).  Records are 27 bytes, unpadded: x, y, z, nx, ny, nz
 *   little-endian float32, then red, green, blue uint8.  x, y, z and the colour are itermvs_fuse_points' (the same device code);
 *   every argument, the workspace, the capacity rule (nothing outside records[0 : 27 * capacity] is written), cursor, view_counts
 *   and the three launches (the same count and scan kernels, an emit kernel of its own; no atomics, no workgroup waits on
 *   another) are as there.
 * The normal of pixel p = (x, y), all in fp64 without fused multiply-add, sums in the written order, IEEE sqrt and division:
 *   1. d = depth_avg[p]; d not finite or d <= 0: the normal is (0,0,0) (the vertex is emitted all the same).
 *   2. Pc(q) = inv(K_ref) (xq*dq, yq*dq, dq): the camera-space point itermvs_fuse_points computes on its way to x, y, z.
 *   3. A neighbour q is usable iff it is inside the image, dq is finite and > 0 and fabs(dq - d) < edge_thres * d (false for
 *      NaN).  It need not be in final_mask: depth_avg is defined at every pixel.  Left / right are tested on the row: x = 0 has no
 *      left and x = W-1 no right neighbour.
 *   4. tx = Pc(x+1,y) - Pc(x-1,y) when both are usable, Pc(x+1,y) - Pc(p) or Pc(p) - Pc(x-1,y) when one is, and the normal is
 *      (0,0,0) when neither is; ty likewise with y+1, y-1.
 *   5. nc = (tx.y*ty.z - tx.z*ty.y, tx.z*ty.x - tx.x*ty.z, tx.x*ty.y - tx.y*ty.x).
 *   6. s = (nc.x*Pc.x + nc.y*Pc.y) + nc.z*Pc.z at p; s > 0: nc = -nc, so the normal faces the camera that saw the point.
 *   7. To world space with the 3x3 part of inv(E_ref), cam[9+0..2], cam[9+4..6], cam[9+8..10] upcast: (m0*a + m1*b) + m2*c.
 *   8. len = sqrt((nx*nx + ny*ny) + nz*nz); len not finite or not > 0: (0,0,0); else each component / len, converted to fp32 once.
 * edge_thres: relative depth step beyond which a neighbour is another surface (eval.py's default 0.01).
 * Validation before the launch: the checks of itermvs_fuse_points, then ITERMVS_ERR_DIMS unless edge_thres is finite and > 0.
 * ------------------------------------------------------------------------------------------ */
int itermvs_fuse_points_normals(const double* depth_avg, const uint8_t* final_mask, const uint8_t* photo_mask,
                                const uint8_t* geo_mask, const float* cam, const uint8_t* rgb, int32_t H, int32_t W,
                                double edge_thres, uint8_t* records, int64_t capacity, uint64_t* cursor,
                                int64_t* view_counts, int32_t view, uint32_t* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * The triangle mesh of a scan (eval.py --mesh; csrc/tsdf.hip, csrc/tsdf_tets.hpp; no counterpart in the reference; numpy
 * restatement: tests/tsdf_reference.py).  A dense volume of nx * ny * nz voxels, voxel (ix, iy, iz) at index (iz*ny + iy)*nx + ix,
 * its centre at c = (ox + (ix + 0.5)*voxel, oy + (iy + 0.5)*voxel, oz + (iz + 0.5)*voxel): the index as fp64, + 0.5, * voxel, + the
 * origin, each rounded once.  All fp64 arithmetic below is without fused multiply-add, sums in the written order, IEEE division.
 * State: device [n][3] uint32 = 12 bytes per voxel, little-endian: sum_t fp32 | count uint16 | red, green, blue sums uint16.  Running
 *   sums, not means.  All zero = empty.  A voxel whose count has reached 257 ignores every further view (257 * 255 = 65535 is the
 *   largest colour sum a uint16 holds), so no field ever wraps.
 *
 * itermvs_tsdf_integrate -- folds V >= 1 views of one size into the volume, ONE launch, one thread per voxel; the thread reads its
 *   state once, walks the views v = 0..V-1 in order and writes the state once.  depth [V][H][W] fp64 and mask [V][H][W] uint8 are
 *   depth_avg and photo && geo of itermvs_fuse_depth; cams [V][21] fp32 = K (9, row-major) | rows 0..2 of E (12), world -> camera;
 *   rgb [V][H][W][3] uint8.  Per voxel and view, with K and E upcast to fp64:
 *   1. count == 257: skip.
 *   2. pc.x = ((e0*c.x + e1*c.y) + e2*c.z) + e3, pc.y and pc.z with e4..7 and e8..11.  pc.z not finite or <= 0: skip.
 *   3. u.x = ((k0*pc.x + k1*pc.y) + k2*pc.z) / pc.z, u.y with k3..5 (row 2 of K is taken to be 0 0 1).
 *   4. px = rint(u.x), py = rint(u.y) (ties to even); unless 0 <= px <= W-1 and 0 <= py <= H-1, compared in fp64 (NaN, inf fail): skip.
 *   5. mask[v][py][px] == 0: skip.  d = depth[v][py][px] not finite or <= 0: skip.
 *   6. sdf = d - pc.z; sdf < -trunc: skip (hidden behind the surface).
 *   7. t = fmin(1, sdf / trunc) in fp64, converted to fp32 once; sum_t += t in fp32; the three colour sums += rgb[v][py][px]; ++count.
 *   No atomics, nothing depends on scheduling; the same views in batches of any size, in the same order, give the same bits.
 *   Validation before the launch, in this order: ITERMVS_ERR_NULL for a NULL pointer; ITERMVS_ERR_DIMS for nx, ny or nz < 1, for
 *   nx*ny*nz beyond the flat bound (2^32 - 256 voxels, csrc/flat_launch.hpp), for voxel not finite or not > 0 or a non-finite origin,
 *   for trunc not finite or not > 0, for V, H or W < 1 and for H*W > 2^31 - 1.
 *
 * itermvs_tsdf_mesh -- marching tetrahedra over the cells; a cell is the cube of the 8 voxel centres (ix..ix+1, iy..iy+1, iz..iz+1)
 *   and carries the index of its corner 0 (ix, iy, iz); corner bit 0 = +x, bit 1 = +y, bit 2 = +z.
 *   1. A voxel is valid iff count >= min_count (>= 1); its value is f = sum_t / (float)count in fp32; it is inside iff f < 0 (0 is outside).
 *   2. A cell is valid iff all 8 corners are valid.  It is cut into the six tetrahedra of the Freudenthal (Kuhn) triangulation,
 *      tetrahedron 0..5 = the axis orders xyz, xzy, yxz, yzx, zxy, zyx, as cube corners {0,1,3,7} {0,5,1,7} {0,3,2,7} {0,2,6,7} {0,4,5,7}
 *      {0,6,4,7} (all positively oriented), and each tetrahedron emits the 0, 1 or 2 triangles of its 4-bit inside mask by the rule in
 *      csrc/tsdf_tets.hpp (itermvs_tsdf_tet_corners and itermvs_tsdf_tet_case fill in both tables; the latter returns the number of triangles).  Triangles are counter-clockwise seen
 *      from the positive side.
 *   3. A vertex exists for (voxel a, direction) iff a valid cell has that edge and its two ends differ in inside.  Directions
 *      0..6 = +x, +y, +z, +xy, +xz, +yz, +xyz lead to the neighbour b.  With fa, fb the fp32 values: s = (double)fa / ((double)fa -
 *      (double)fb); each coordinate is ca + s * (cb - ca) from the two centres' coordinates, converted to fp32 once; each colour
 *      channel is qa + s * (qb - qa) with q = (double)sum / (double)count, then rint, clamped to 0..255, converted to uint8.
 *   4. Vertices are numbered in ascending (voxel index, direction); triangles in ascending (cell index, tetrahedron, triangle of the case).
 *   vertices: `vertex_capacity` records of 15 bytes, unpadded (x, y, z little-endian float32; red, green, blue uint8); faces:
 *   `face_capacity` triples of int32 vertex indices.  A vertex or triangle whose number is >= its capacity is not stored; totals
 *   (device uint64 [2] = vertices, triangles) holds the true totals all the same, so the caller sees the overflow.  The stored
 *   triangles always hold the true vertex numbers.  Nothing outside vertices[0 : 15*vertex_capacity], faces[0 : 3*face_capacity],
 *   totals and the workspace is written.  One memset and five launches (mark, count, one-workgroup scan, vertex, face); the marks
 *   are plain byte stores of the constant 1; no atomics, no workgroup waits on another.
 *   workspace: the *bytes of itermvs_tsdf_mesh_workspace_bytes(nx, ny, nz, bytes) (16 per 256 voxels + 12 per voxel), 8-byte aligned.
 *   Validation before any HIP call: ITERMVS_ERR_NULL for NULL state, totals, workspace, or NULL vertices / faces with a capacity
 *   other than 0; ITERMVS_ERR_DIMS as for the volume above, for min_count < 1, a capacity < 0 and vertex_capacity > 2^31 - 1;
 *   ITERMVS_ERR_ALIGN for the workspace.
 * ------------------------------------------------------------------------------------------ */
int itermvs_tsdf_tet_corners(int32_t tet, int32_t* corners /* host [4] */);
int itermvs_tsdf_tet_case(int32_t mask, int32_t* edges /* host [12]: triangle t, vertex v = local corners [6t+2v], [6t+2v+1]; -1 beyond */);
int itermvs_tsdf_integrate(uint32_t* state, int32_t nx, int32_t ny, int32_t nz, double ox, double oy, double oz, double voxel,
                           double trunc, const double* depth, const uint8_t* mask, const float* cams, const uint8_t* rgb,
                           int32_t V, int32_t H, int32_t W, void* stream);
int itermvs_tsdf_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int64_t* bytes /* host */);
int itermvs_tsdf_mesh(const uint32_t* state, int32_t nx, int32_t ny, int32_t nz, double ox, double oy, double oz, double voxel,
                      int32_t min_count, uint8_t* vertices, int64_t vertex_capacity, int32_t* faces, int64_t face_capacity,
                      uint64_t* totals, uint8_t* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Connected components of an indexed triangle mesh and the compaction of the components worth keeping (eval.py
 * --mesh_min_component / --mesh_component_share, clean_mesh.py; csrc/mesh_components.hip; no counterpart in the reference; numpy
 * restatement: tests/mesh_components_reference.py).  Integers only: every output is determined by the inputs bit for bit, whatever
 * the scheduling.  faces: device [NF][3] int32 vertex indices.  A face is VALID iff all three indices lie in [0, NV); an invalid
 * face is ignored everywhere (not united, not counted, not emitted), like an out-of-range entry of the COLMAP kernels below.
 * Degenerate faces (a, a, b) and duplicate faces are valid and count.
 *
 * itermvs_mesh_components -- label, face_count: device [NV] int32; totals: device uint64 [3].
 *   1. Two vertices are connected iff a chain of valid faces links them; sharing ONE vertex index is enough.
 *   2. label[v] = the smallest vertex index of v's component; a vertex that no valid face references has label[v] = v.
 *   3. face_count[r] = the number of valid faces whose vertices carry label r, stored where label[r] == r; 0 everywhere else.
 *   4. totals = the number of components with at least one face | the largest face_count | the number of valid faces.
 *   A memset of totals and five launches (init, hook, flatten, count, totals; hook and count are skipped for NF == 0): a lock-free
 *   union-find whose one hooking store is a compare-and-swap at a root that hangs the larger root under the smaller, so a parent only
 *   ever decreases and every walk and every retry ends by construction; integer atomicMin / atomicCAS / atomicAdd / atomicMax at
 *   agent scope; no thread waits on another thread's progress, the host is not asked between the launches.
 *   Validation before any HIP call: ITERMVS_ERR_NULL for NULL label, face_count or totals, and for NULL faces unless NF == 0;
 *   ITERMVS_ERR_DIMS for NV < 0, NF < 0 and NF > 2^31 - 1 (the int32 limit of csrc/flat_launch.hpp: a face_count never wraps).
 *   NV == 0 and NF == 0 are legal: totals is written, for NV == 0 nothing else.
 *
 * itermvs_mesh_keep -- vertices: device [NV] records of record_bytes (1..64; the mesh's is 15) bytes, unpadded; label, face_count as
 *   itermvs_mesh_components wrote them for `faces`.
 *   1. A vertex v is kept iff face_count[label[v]] >= min_faces (>= 1); a vertex that no valid face references therefore goes.
 *      (A label outside [0, NV) keeps nothing.)
 *   2. A face is kept iff it is valid and its first vertex is kept (its other two carry the same label).
 *   3. out_vertices: the kept records, unchanged, in ascending v.  out_faces: the kept faces in ascending order, each index replaced
 *      by its vertex's rank among the kept vertices.
 *   Capacities and totals (device uint64 [2] = kept vertices, kept faces) as for itermvs_tsdf_mesh: a vertex or face whose number is
 *   >= its capacity is not stored, totals holds the true counts all the same, the stored faces hold the true new indices; nothing
 *   outside out_vertices[0 : record_bytes*vertex_capacity], out_faces[0 : 3*face_capacity], totals and the workspace is written.
 *   Five launches (mark + per-256 count of the vertices, per-256 count of the faces, one-workgroup scan, vertex scatter, face
 *   scatter; the face launches are skipped for NF == 0); no atomics, no workgroup waits on another.
 *   workspace: the *bytes of itermvs_mesh_keep_workspace_bytes(NV, NF, bytes) (8 per 256 vertices and per 256 faces + 5 per vertex,
 *   rounded up to 8), 8-byte aligned.
 *   Validation before any HIP call: ITERMVS_ERR_NULL for NULL label, face_count, totals or workspace, NULL vertices unless NV == 0,
 *   NULL faces unless NF == 0, NULL out_vertices / out_faces with a capacity other than 0; ITERMVS_ERR_DIMS for the sizes as above,
 *   record_bytes outside 1..64, min_faces < 1, a capacity < 0 and vertex_capacity > 2^31 - 1; ITERMVS_ERR_ALIGN for the workspace.
 * ------------------------------------------------------------------------------------------ */
int itermvs_mesh_components(const int32_t* faces, int64_t NF, int32_t NV, int32_t* label, int32_t* face_count, uint64_t* totals,
                            void* stream);
int itermvs_mesh_keep_workspace_bytes(int32_t NV, int64_t NF, int64_t* bytes /* host */);
int itermvs_mesh_keep(const uint8_t* vertices, int32_t NV, int32_t record_bytes, const int32_t* faces, int64_t NF, const int32_t* label,
                      const int32_t* face_count, int32_t min_faces, uint8_t* out_vertices, int64_t vertex_capacity, int32_t* out_faces,
                      int64_t face_capacity, uint64_t* totals, uint8_t* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Simplification of an indexed triangle mesh by vertex clustering with quadric placement (eval.py --mesh_simplify, simplify_mesh.py;
 * csrc/mesh_simplify.hip; Lindstrom 2000, "Out-of-core simplification of large polygonal models"; no counterpart in the reference;
 * numpy restatement: tests/mesh_simplify_reference.py; host side: itermvs_amd/fusion.py simplify_mesh).  Additions compatible with
 * ABI 20.  vertices: device [NV] records of record_bytes (12..64; the mesh's is 15) bytes, unpadded; bytes 0..11 are float32 x, y, z,
 * little-endian; a record of at least 15 bytes has red, green, blue in bytes 12..14.  faces: device [NF][3] int32.  The grid (origin
 * ox, oy, oz; nx, ny, nz cells of side `cell`) and its key are those of itermvs_cloud_cell_keys below.  All arithmetic is fp64 on the
 * float32 coordinates without contraction, sums are taken in the written order, division is IEEE; no float atomics, no workgroup
 * waits on another, the host is not asked between the launches: the same input gives the same bytes on every run.
 *   1. A vertex is VALID iff its three coordinates are finite and it lies inside the grid (its key is not INT64_MAX).
 *   2. A face is VALID iff its three indices lie in [0, NV) and its three vertices are valid.
 *   3. A cluster is the set of valid vertices of one cell.  Clusters are numbered in ascending cell key; inside a cluster the members
 *      are in ascending vertex index.
 *   4. The representative of a cluster with m members.  m == 1: the member's record, all record_bytes unchanged.  m > 1:
 *      mu.x = sx / (double)m with sx = 0.0; sx = sx + x_k over the members in order (y, z alike).  record_bytes >= 15: each colour
 *      channel is rint((double)(integer sum over the members) / (double)m) as uint8.  Every other byte from the 12th on is copied
 *      from the lowest member.  Over every valid face with at least one corner in the cluster, once each, in ascending face index,
 *      with a, b, c its three ORIGINAL positions, u = b - a, v = c - a:
 *        n.x = (u.y*v.z) - (u.z*v.y); n.y = (u.z*v.x) - (u.x*v.z); n.z = (u.x*v.y) - (u.y*v.x)   (unnormalised: weight = area^2)
 *        h = ((n.x*(a.x - mu.x)) + (n.y*(a.y - mu.y))) + (n.z*(a.z - mu.z))
 *        Axx += n.x*n.x; Axy += n.x*n.y; Axz += n.x*n.z; Ayy += n.y*n.y; Ayz += n.y*n.z; Azz += n.z*n.z;
 *        r.x += n.x*h; r.y += n.y*h; r.z += n.z*h                                              (all nine sums start at 0.0)
 *      trace = (Axx + Ayy) + Azz; lambda = ITERMVS_MESH_SIMPLIFY_REG * trace (1e-3: a choice of Lindstrom's order of magnitude, not
 *      a measured optimum); a00 = Axx + lambda, a11 = Ayy + lambda, a22 = Azz + lambda; the cofactors
 *        c00 = (a11*a22) - (Ayz*Ayz); c01 = (Axz*Ayz) - (Axy*a22); c02 = (Axy*Ayz) - (Axz*a11);
 *        c11 = (a00*a22) - (Axz*Axz); c12 = (Axy*Axz) - (a00*Ayz); c22 = (a00*a11) - (Axy*Axy);
 *      det = ((a00*c00) + (Axy*c01)) + (Axz*c02);
 *        y.x = (((c00*r.x) + (c01*r.y)) + (c02*r.z)) / det; y.y = (((c01*r.x) + (c11*r.y)) + (c12*r.z)) / det;
 *        y.z = (((c02*r.x) + (c12*r.y)) + (c22*r.z)) / det.
 *      y = 0 if trace == 0, if det is not finite or not > 0, or if a component of y is not finite.  Per axis, with i the cell's
 *      index on it, lo = o + (double)i*cell, hi = o + (double)(i + 1)*cell: x = mu + y; x < lo ? lo : (x > hi ? hi : x), converted
 *      to float32 once.
 *   5. A valid face becomes its three cluster numbers in its own corner order.  It is dropped if two of them are equal, or if an
 *      earlier surviving face has the same triple up to cyclic rotation (the same orientation; the opposite orientation is another
 *      face and stays).  Survivors stay in ascending original face index.
 *   6. The output vertices are the representatives of the clusters that a surviving face references, in ascending cluster number;
 *      the faces are renumbered to match.  No unreferenced vertex is written.
 * The sorts between the entry points are the caller's and must be STABLE (itermvs_amd/fusion.py simplify_mesh: torch.sort):
 *   keys_sorted, perm: the vertices' keys ascending and perm int64 [NV] = the vertex at each sorted position; cluster_sorted int32
 *   [NV] = the inclusive prefix sum of itermvs_cloud_voxel_heads(keys_sorted) minus 1, or -1 where the key is INT64_MAX; cluster int32
 *   [NV] = the same per vertex (cluster[perm[i]] = cluster_sorted[i]).
 *
 * itermvs_mesh_simplify_corners -- one launch.  pair_cluster int32 [NF][3] = the cluster of each corner of a valid face, 2^31 - 1
 *   three times for an invalid one.  A face is ALIVE iff it is valid and its three clusters differ; its canonical triple (c0, c1, c2)
 *   is the cyclic rotation that starts at the smallest.  key_hi int64 [NF] = (c0 << 32) | c1, INT64_MAX unless alive; key_lo int32
 *   [NF] = c2, 2^31 - 1 unless alive.  The caller sorts the 3*NF pairs (pair_cluster flat, index e = 3*face + corner: face-major)
 *   by cluster into pair_sorted and pair_face[e] = the face of the pair now at e, and the faces by (key_hi, key_lo) into
 *   key_hi_sorted, key_lo_sorted and order int32 [NF] = the face at each sorted position.
 * itermvs_mesh_simplify_clusters -- one launch, rule 4: reps: device [NV] records; record c is the representative of cluster c (the
 *   records from the number of clusters on are not written).  The thread at the head of each run of cluster_sorted walks the run and
 *   then the cluster's run of pair_sorted, found by binary search, skipping a pair whose face equals the pair's before it.
 * itermvs_mesh_simplify_emit -- rules 5 and 6.  A memset of the marks and six launches (mark: the head of each run of equal sorted
 *   triples survives and marks its three clusters, plain byte stores of the constant 1; per-256 count of the clusters, of the faces;
 *   one-workgroup scan; vertex scatter; face scatter).  Capacities and totals (device uint64 [2] = vertices, faces) as for
 *   itermvs_tsdf_mesh: a vertex or face whose number is >= its capacity is not stored, totals holds the true counts all the same, the
 *   stored faces hold the true new indices; nothing outside out_vertices[0 : record_bytes*vertex_capacity], out_faces[0 :
 *   3*face_capacity], totals and the workspace is written.  workspace: the *bytes of itermvs_mesh_simplify_emit_workspace_bytes(NV,
 *   NF, bytes) (8 per 256 vertices and per 256 faces + 5 per vertex + 1 per face, rounded up to 8), 8-byte aligned.
 * Validation before any HIP call, all three: ITERMVS_ERR_NULL for a NULL pointer (the per-vertex arrays may be NULL iff NV == 0, the
 *   per-face arrays iff NF == 0, out_vertices / out_faces iff their capacity is 0; totals and workspace never); ITERMVS_ERR_DIMS for
 *   NV < 0, NF < 0, NF > (2^31 - 1) / 3 (the pairs are indexed in an int32), record_bytes outside 12..64, cell not finite or not > 0,
 *   a non-finite origin, a grid dimension outside 1..2^21, a capacity < 0 and vertex_capacity > 2^31 - 1; ITERMVS_ERR_ALIGN for the
 *   workspace.  NV == 0 and NF == 0 are legal: emit writes totals = {0, 0} and nothing else.  No content of a mesh (NaN or huge
 *   coordinates, indices of -1 or 2^31 - 1) makes a kernel read or write outside its buffers, and every index taken from one of the
 *   caller's arrays is compared with its range before use: arrays that do not describe the mesh give a wrong mesh, nothing worse.
 * ------------------------------------------------------------------------------------------ */
#define ITERMVS_MESH_SIMPLIFY_REG 1e-3
int itermvs_mesh_simplify_corners(const int32_t* faces, int64_t NF, int32_t NV, const int32_t* cluster, int32_t* pair_cluster,
                                  int64_t* key_hi, int32_t* key_lo, void* stream);
int itermvs_mesh_simplify_clusters(const uint8_t* vertices, int32_t NV, int32_t record_bytes, const int32_t* faces, int64_t NF,
                                   const int64_t* keys_sorted, const int64_t* perm, const int32_t* cluster_sorted,
                                   const int32_t* pair_sorted, const int32_t* pair_face, double ox, double oy, double oz, int32_t nx,
                                   int32_t ny, int32_t nz, double cell, uint8_t* reps, void* stream);
int itermvs_mesh_simplify_emit_workspace_bytes(int32_t NV, int64_t NF, int64_t* bytes /* host */);
int itermvs_mesh_simplify_emit(const uint8_t* reps, int32_t NV, int32_t record_bytes, const int32_t* faces, int64_t NF,
                               const int32_t* cluster, const int64_t* key_hi_sorted, const int32_t* key_lo_sorted, const int32_t* order,
                               uint8_t* out_vertices, int64_t vertex_capacity, int32_t* out_faces, int64_t face_capacity,
                               uint64_t* totals, uint8_t* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * The COLMAP converter's two device stages (csrc/colmap.hip; colmap_input.py of the reference, host side: itermvs_amd/colmap.py).
 * Common inputs (device): the images' observation lists as CSR -- offsets [V+1] int64 ascending, point [offsets[V]] int32 = dense
 *   point index into xyz or -1, in file order (image index = position in images.bin) -- and xyz [P][3] fp64.  An entry outside
 *   [0, P) is ignored like -1.  Validation before launch: ITERMVS_ERR_NULL for a NULL pointer, ITERMVS_ERR_DIMS for V < 1 or
 *   P < 1; that offsets ascend and end inside `point` is the caller's duty (itermvs_amd.ops checks it on the host).  Neither
 *   entry point allocates or synchronises; one launch each.
 *
 * itermvs_view_scores -- calc_score and the pair loop (colmap_input.py:336-364).  centre [V][3] fp64 = -R^T t.  For i < j,
 *   score[i][j] = score[j][i] = sum over the entries pid of image i's list (list order, WITH multiplicity, -1 skipped) that occur
 *   in image j's list of exp(-(th - theta0)^2 / (2 s^2)), th = (180 / pi) acos(<ci - p, cj - p> / |ci - p| / |cj - p|) in degrees,
 *   s = sigma1 if th <= theta0 else sigma2.  score [V][V] fp64: EVERY element is written (diagonal 0, pairs without a common
 *   point exactly 0, bitwise symmetric).  All arithmetic fp64 without fused multiply-add.  Each pair is summed by one wave in a
 *   fixed shape (lane t takes entries t, t + 64, ..; a fixed shuffle tree), without floating-point atomics: two runs on the same
 *   input give the same bits.  Membership is a bitmap of image j's points in LDS, 524288 points per chunk; larger P is walked
 *   chunk by chunk and the chunks' sums are added in ascending order.
 *   Unlike the reference the cosine is clamped to [-1, 1] (np.arccos returns NaN for a cosine that rounded above 1).
 *
 * itermvs_depth_ranges -- colmap_input.py:319-333.  ext_row2 [V][4] fp64 = row 2 of each extrinsic.  With
 *   zs = sorted(((e0 x + e1 y) + e2 z) + e3 over the image's valid observations, a repeated point counting twice; no FMA):
 *   range[v] = {zs[int(len * .01)], zs[int(len * .99)]}: exact order statistics (8-pass radix select; the result is one of the
 *   z values bit for bit), no interpolation.  range [V][2] fp64.  An image without a valid observation gets {NaN, NaN} (the
 *   reference raises IndexError at :330; the host raises ValueError).
 * ------------------------------------------------------------------------------------------ */
int itermvs_view_scores(const int64_t* offsets, const int32_t* point, const double* xyz, const double* centre, int32_t V,
                        int32_t P, double theta0, double sigma1, double sigma2, double* score, void* stream);
int itermvs_depth_ranges(const int64_t* offsets, const int32_t* point, const double* xyz, const double* ext_row2, int32_t V,
                         int32_t P, double* range, void* stream);

/* ------------------------------------------------------------------------------------------
 * The searches of the DTU point-cloud evaluation (csrc/cloud_eval.hip; the .m scripts under evaluations/dtu of the reference, host side:
 * itermvs_amd/cloud_eval.py).  Clouds are float32 [n][3] (PLY coordinates); all arithmetic is fp64 on them, the squared distance
 * is ((dx*dx) + (dy*dy)) + (dz*dz) without contraction and the distance its IEEE sqrt.
 * The neighbour structure is a uniform grid (origin ox, oy, oz; nx, ny, nz cells of edge `edge`): cell = floor((p - origin) / edge),
 * key = (cx * ny + cy) * nz + cz.  Validation before any launch, common to all: ITERMVS_ERR_NULL for a NULL pointer;
 * ITERMVS_ERR_DIMS for a point count < 1 or > 0x7fffff00, a non-finite origin, edge <= 0, or a grid dimension outside
 * 1 .. 2^21 (a cloud whose extent does not fit the 63-bit key).  No entry point allocates or synchronises; one launch each.
 * No content of a cloud (NaN, Inf, huge coordinates) makes a kernel read or write outside its buffers.
 *
 * itermvs_cloud_cell_keys: keys[i] = the key of point i; INT64_MAX for a point that is not finite or lies outside the grid.  The
 *   caller sorts by key (the sorted arrays below are the points / keys / ranks in that order).
 *
 * itermvs_cloud_reduce_round -- one round of reducePts_haa.m:24-30 (the loop `if indexSet(id), indexSet(idx{i}) = 0,
 *   indexSet(id) = 1` over rangesearch(..., dst), d2 <= dst*dst inclusive).  rank_sorted[i] = position of point i in the
 *   visiting order (RandOrd).  state [n] int32, zeroed by the caller before the first round: 0 undecided, 1 kept, 2 removed.
 *   An undecided point becomes removed if a neighbour of lower rank is kept, kept if no neighbour of lower rank is undecided;
 *   *undecided (device int32, zeroed by the caller) is incremented for every point the round leaves undecided.  Repeating the
 *   round until that count is 0 gives exactly the sequential loop's indexSet for the same order, in at most n rounds.
 *   Needs edge >= dst (ITERMVS_ERR_DIMS otherwise, or for dst <= 0): the 27 cells around a point must hold the radius.
 *
 * itermvs_cloud_nn_distance -- MaxDistCP.m.  region (HOST memory) = {lo[3], hi[3]}: the queries the script's blocks cover,
 *   lo[a] <= x < hi[a] with lo = BB(1,:), hi = (BB(1,:) + floor((BB(2,:) - BB(1,:)) / cap) * cap) + cap.  Queries: q_from [nq][3],
 *   all of them or, with index != NULL, the n_index entries of index (int64, entries outside [0, nq) are skipped).  Targets:
 *   to_sorted [nt][3] with keys_sorted on the given grid.  Per query, carried between calls on successively coarser grids:
 *   best_d2 (fp64, +Inf before the first call), done (uint8, 0 before the first call; a done query is skipped).  A call searches
 *   the rings 0 .. rings - 1 of cells around the query's cell, stops as soon as best_d2 <= ((r - 1) * edge * (1 - 2^-20))^2 or
 *   that bound >= cap, and sets done when it stopped that way.  dist = min(sqrt(best_d2), cap); cap (and done) at once for a
 *   query outside the region.  When done is set, dist = min(distance to the nearest target, cap) over ALL targets on the grid.
 *   Unlike MaxDistCP.m, which returns the distance to the nearest point of the block enlarged by cap (possibly > cap: every
 *   consumer discards >= 20), and without the one-ulp seams between neighbouring blocks' Low / High.
 *   ITERMVS_ERR_DIMS also for cap <= 0, rings outside 1 .. 2^21, n_index outside 1 .. nq.
 *
 * itermvs_cloud_in_mask -- PointCompareMain.m:32-41.  out[i] = 1 iff v = round(((p - b) / res) + 1) (half away from zero, per
 *   axis) lies in 1 .. (sx, sy, sz) and mask[vx - 1][vy - 1][vz - 1] != 0; mask is uint8 [sx][sy][sz] contiguous.
 *   ITERMVS_ERR_DIMS for a size < 1, res <= 0 or a non-finite b / res.
 * ------------------------------------------------------------------------------------------ */
int itermvs_cloud_cell_keys(const float* xyz, int64_t n, double ox, double oy, double oz, int32_t nx, int32_t ny, int32_t nz,
                            double edge, int64_t* keys, void* stream);
int itermvs_cloud_reduce_round(const float* xyz_sorted, const int64_t* keys_sorted, const int32_t* rank_sorted, int64_t n,
                               double ox, double oy, double oz, int32_t nx, int32_t ny, int32_t nz, double edge, double dst,
                               int32_t* state, int32_t* undecided, void* stream);
int itermvs_cloud_nn_distance(const float* q_from, int64_t nq, const int64_t* index, int64_t n_index, const float* to_sorted,
                              const int64_t* keys_sorted, int64_t nt, double ox, double oy, double oz, int32_t nx, int32_t ny,
                              int32_t nz, double edge, const double* region, double cap, int32_t rings, double* best_d2,
                              uint8_t* done, double* dist, void* stream);
int itermvs_cloud_in_mask(const float* xyz, int64_t n, const uint8_t* mask, int32_t sx, int32_t sy, int32_t sz, double bx,
                          double by, double bz, double res, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The point-cloud passes of the Tanks and Temples evaluation (csrc/cloud_register.hip; host side: itermvs_amd/cloud_register.py).
 * Additions compatible with ABI 18.  Clouds are float32 [n][3]; all arithmetic is fp64 on them without contraction.  T is a 4x4
 * fp64 row-major matrix in HOST memory (rows 0..2 are used; identity = no transform), applied per row as
 * ((m0*x + m1*y) + m2*z) + m3.  Every check precedes the first launch: ITERMVS_ERR_NULL for a NULL pointer, ITERMVS_ERR_DIMS for a
 * point count < 1 or > 0x7fffff00, a non-finite T, and what each entry adds.  Nothing allocates or synchronises; no float atomics:
 * the same input gives the same bytes on every run.
 *
 * itermvs_cloud_crop -- replaces Open3D's SelectionPolygonVolume.crop_point_cloud.  out[i] = 1 iff c = T * p_i lies in the volume:
 *   axis w in {0, 1, 2} is the orthogonal axis, axis_min <= c_w <= axis_max (inclusive), and (c_u, c_v) is inside the polygon by
 *   the even-odd rule, (u, v) = (1, 2) for w = 0 (X), (0, 2) for w = 1 (Y), (0, 1) for w = 2 (Z).  polygon: HOST memory, fp64
 *   [n_poly][3] vertices (only u and v are read), 3 <= n_poly <= 1024.  With a = vertex k and b = vertex k + 1 (the last edge
 *   closes the polygon), edge (a, b) toggles iff (a_v > c_v) != (b_v > c_v) and
 *   c_u < (((b_u - a_u) * (c_v - a_v)) / (b_v - a_v)) + a_u, in exactly this order of operations.  A point whose c is not finite
 *   is outside.  poly_ws: device scratch of 2 * n_poly doubles (the polygon travels there as kernel arguments, 128 vertices per
 *   launch, before the crop launch on the same stream).  ITERMVS_ERR_DIMS also for an axis outside 0..2, n_poly outside 3..1024,
 *   a NaN bound or a non-finite polygon coordinate.
 *
 * itermvs_cloud_voxel_heads / itermvs_cloud_voxel_mean -- replace Open3D's voxel_down_sample: one output point per occupied
 *   voxel, the mean of its members.  The caller computes the keys with itermvs_cloud_cell_keys (origin = min_bound - voxel / 2,
 *   edge = voxel) and sorts them STABLY.  voxel_heads: head[i] (int32) = 1 iff keys_sorted[i] != INT64_MAX and i is the first of
 *   its run of equal keys.  The caller's inclusive prefix sum of head, minus 1, is rank (int64 [n]; torch.cumsum: plumbing), its
 *   last element + 1 is n_out.  voxel_mean: the head of every run adds the run's coordinates in sorted order -- original index
 *   order inside a voxel -- in fp64 starting from 0.0, divides by the count and rounds once to float32 into out[rank][3]; a rank
 *   outside [0, n_out) writes nothing.  Output order: ascending voxel key (Open3D's is a hash map's).  Runs longer than 64 points
 *   are summed by the whole wave from coalesced loads, in the same order and therefore to the same bits.
 *   ITERMVS_ERR_DIMS also for n_out outside 1 .. n.
 *
 * itermvs_cloud_nn_index -- replaces the KD-tree correspondence search of Open3D's registration_icp.  For every query
 *   T * q_i: the nearest target of to_sorted (key order on the given grid, keys_sorted as for itermvs_cloud_nn_distance) with
 *   d2 < max_dist * max_dist.  The bound is EXCLUSIVE: a target exactly max_dist away is no match.  idx[i] = perm[position] (perm:
 *   int64 [nt], the sorted position's index in the caller's unsorted target array) or -1; d2[i] = the squared distance (fp64) or
 *   +Inf.  Ties on d2 go to the lowest perm value, whatever the traversal order.  The search walks the rings 0 .. rings - 1 with
 *   the ring walk and stop bounds of itermvs_cloud_nn_distance (csrc/cloud_grid.hpp); rings >= the first ring whose lower bound
 *   (r - 1) * edge * (1 - 2^-20) reaches max_dist makes the result exact.  nt = 0 is allowed (every query unmatched; the target
 *   pointers may then be NULL).  ITERMVS_ERR_DIMS also for nt < 0, a bad grid, max_dist <= 0, rings outside 1 .. 2^21.
 *
 * itermvs_cloud_umeyama_sums -- replaces the sums inside Open3D's TransformationEstimationPointToPoint (Eigen::umeyama).  Over the
 *   correspondences with 0 <= idx[i] < nt, p = T * q_i, t = target[idx[i]] (the UNSORTED targets): sums[18] = {count, sum p (3),
 *   sum t (3), sum t p^T (9, row = t, column = p), sum ((px*px + py*py) + pz*pz), sum d2[i]}.  Fixed-shape reduction:
 *   G = itermvs_cloud_umeyama_groups(n) = min(1024, ceil(n / 2048)) workgroups of 256 threads; workgroup g owns the slice
 *   [g * S, (g + 1) * S), S = ceil(n / G); thread t adds elements t, t + 256, ... in order; lanes combine by xor-butterfly
 *   (32, 16, ..., 1), the 4 waves in wave order -> partials[g][18] (device, G * 18 doubles); one workgroup adds the partials in
 *   ascending g -> sums (device, 18 doubles).  ITERMVS_ERR_DIMS also for nt < 0.
 * ------------------------------------------------------------------------------------------ */
int itermvs_cloud_crop(const float* xyz, int64_t n, const double* T, int32_t axis, double axis_min, double axis_max,
                       const double* polygon, int32_t n_poly, double* poly_ws, uint8_t* out, void* stream);
int itermvs_cloud_voxel_heads(const int64_t* keys_sorted, int64_t n, int32_t* head, void* stream);
int itermvs_cloud_voxel_mean(const float* xyz_sorted, const int64_t* keys_sorted, const int64_t* rank, int64_t n, int64_t n_out,
                             float* out, void* stream);
int itermvs_cloud_nn_index(const float* q, int64_t nq, const double* T, const float* to_sorted, const int64_t* keys_sorted,
                           const int64_t* perm, int64_t nt, double ox, double oy, double oz, int32_t nx, int32_t ny, int32_t nz,
                           double edge, double max_dist, int32_t rings, int64_t* idx, double* d2, void* stream);
int itermvs_cloud_umeyama_groups(int64_t n);
int itermvs_cloud_umeyama_sums(const float* q, int64_t n, const double* T, const int64_t* idx, const double* d2,
                               const float* target, int64_t nt, double* partials, double* sums, void* stream);

/* ------------------------------------------------------------------------------------------
 * Outlier removal of a fused cloud (csrc/cloud_filter.hip; host side: itermvs_amd/cloud_filter.py).  Additions compatible with
 * ABI 20.  The queries are the targets: xyz_sorted float32 [n][3] / keys_sorted int64 [n] are ONE cloud in key order on the given
 * grid (itermvs_cloud_cell_keys, sorted by the caller), perm int64 [n] the sorted position's index in the caller's unsorted cloud;
 * outputs are written at perm[position], that is in the caller's order (a perm value outside [0, n) writes nothing).  One lane per
 * sorted position.  Arithmetic: fp64 on the float32 coordinates, d2 = ((dx*dx) + (dy*dy)) + (dz*dz) without contraction.  A query
 * skips its own sorted position and nothing else: another point at distance 0 is a neighbour.  A point with key INT64_MAX (a
 * non-finite coordinate, or outside the grid) is nobody's neighbour and, as a query, gets flag 1 / count 0.  Checks before any
 * launch: ITERMVS_ERR_NULL for a NULL pointer (index excepted), ITERMVS_ERR_DIMS for the grid errors of the searches above and
 * what each entry adds.  No atomics, no LDS, nothing allocates or synchronises; one launch each.
 *
 * itermvs_cloud_knn_mean -- the mean distance to the k nearest other points (Open3D remove_statistical_outlier, PCL
 *   StatisticalOutlierRemoval), limited to `cap`.  Queries: every sorted position or, with index != NULL, the n_index sorted
 *   positions of index (int64; entries outside [0, n) are skipped).  The call walks the rings 0 .. rings - 1 of cells around the
 *   query's cell (csrc/cloud_grid.hpp) keeping the k smallest d2, ascending d2_1 <= ... <= d2_k (+Inf until found), and stops
 *   before ring r >= 1 as soon as d2_k <= lb * lb or lb >= cap, lb = (r - 1) * edge * (1 - 2^-20).  Stopped that way:
 *     isolated <=> !(d2_k <= cap * cap)  (the product rounded once): fewer than k other points within cap.  flag 1, mean +Inf.
 *     otherwise flag 0, mean = (((0.0 + sqrt(d2_1)) + sqrt(d2_2)) + ... + sqrt(d2_k)) / k, IEEE sqrt, added in ascending order.
 *   Rings used up first: flag 2, mean +Inf -- the caller repeats the query on a coarser grid from the start; no state is carried.
 *   Flags 0 and 1 and the mean do not depend on the grid.  mean fp64 [n], flag uint8 [n].
 *   ITERMVS_ERR_DIMS also for k outside 1 .. 32, n <= k, cap not finite or <= 0, rings outside 1 .. 2^21, n_index outside 1 .. n.
 *
 * itermvs_cloud_radius_count -- PCL RadiusOutlierRemoval's count.  count[perm[i]] (int32) = min(number of other points with
 *   d2 <= r * r (the product rounded once, inclusive), limit).  The walk's cap is r: it ends when the ring bound reaches r, or one
 *   ring after `limit` neighbours are counted.  ITERMVS_ERR_DIMS also for r not finite or <= 0, limit < 1, and a grid whose
 *   edge needs more than 64 rings to reach r ((r_ring - 1) * edge * (1 - 2^-20) >= r first at r_ring > 64).
 * ------------------------------------------------------------------------------------------ */
int itermvs_cloud_knn_mean(const float* xyz_sorted, const int64_t* keys_sorted, const int64_t* perm, int64_t n,
                           const int64_t* index, int64_t n_index, double ox, double oy, double oz, int32_t nx, int32_t ny,
                           int32_t nz, double edge, int32_t k, double cap, int32_t rings, double* mean, uint8_t* flag,
                           void* stream);
int itermvs_cloud_radius_count(const float* xyz_sorted, const int64_t* keys_sorted, const int64_t* perm, int64_t n, double ox,
                               double oy, double oz, int32_t nx, int32_t ny, int32_t nz, double edge, double r, int32_t limit,
                               int32_t* count, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_image_pyramid --the input side of the path: datasets/dtu_yao_eval.py:61-74
 * (read_img) on the GPU.  src [V,Hs,Ws,3] uint8 interleaved RGB (the decoded images of one sample, same size) ->
 *   level0 [V,3,H,W]       = cv2.resize(2 * src / 255. - 1, (W, H), INTER_LINEAR)   (float32)
 *   level1..3 [V,3,H>>l,W>>l] = cv2.resize(level0, ..., INTER_LINEAR)               (may be NULL: the network reads level 0 only)
 * H and W multiples of 8 when the lower levels are requested.  cv2's algorithm is restated from its published form.
 * ------------------------------------------------------------------------------------------ */
int itermvs_image_pyramid(const uint8_t* src, int32_t V, int32_t Hs, int32_t Ws, int32_t H, int32_t W, float* level0,
                          float* level1, float* level2, float* level3, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_resize_rgb8 -- Pillow's Image.resize((W, H), Image.BILINEAR) of 8-bit RGB images, bit for bit: the vertex colours
 * of the fusion (eval.py:68-74,295 with PIL in cv2's place) from the uint8 upload of the input side.
 *   src [V,Hs,Ws,3] uint8 -> out [V,H,W,3] uint8, out[v] == np.array(Image.fromarray(src[v]).resize((W, H), Image.BILINEAR)).
 * Pillow's 8-bit resample is integer arithmetic on per-axis tables that the caller computes in doubles
 * (itermvs_amd/resize.py) and passes as device memory:
 *   xbounds [W,2] int32: first input column and tap count of every output column; xk [W,KX] int32: the taps with 22
 *   fractional bits (KX >= every count);  ybounds [H,2], yk [H,KY]: the same for the rows.
 *   pass = clip(((1 << 21) + sum(pixel[first + t] * k[t])) >> 22, 0, 255); horizontal first, its uint8 result feeds the
 *   vertical pass.  An axis that keeps its size takes the identity table (count 1, tap 1 << 22).
 * One launch; taps that a table places outside the image are clamped to it.
 * ------------------------------------------------------------------------------------------ */
int itermvs_resize_rgb8(const uint8_t* src, int32_t V, int32_t Hs, int32_t Ws, int32_t H, int32_t W, const int32_t* xbounds,
                        const int32_t* xk, int32_t KX, const int32_t* ybounds, const int32_t* yk, int32_t KY, uint8_t* out,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_undistort_rgb8 -- one image of a COLMAP camera with lens distortion resampled to a pinhole camera (what COLMAP's
 * image_undistorter does before dense stereo; colmap_input.py leaves it to the user).  One launch per image.
 *   src [Hs,Ws,3] uint8 (device) -> out [Ho,Wo,3] uint8 (device); map [Ho,Wo,2] float64 (device) or NULL: (sx, sy) of every
 *   output pixel as computed below, filled or not -- the kernel's sampling decisions, for the tests.
 *   model: COLMAP's camera model id; params: its n_params parameters in COLMAP's order (HOST doubles, copied into the launch);
 *   fx_o, fy_o, cx_o, cy_o: the output pinhole camera.
 * Per output pixel (x, y), all in float64, one rounding per written operation (no fused multiply-add), COLMAP's pixel-centre
 * convention (pixel (0, 0) covers [0, 1) x [0, 1)):
 *   u = ((x + 0.5) - cx_o) / fx_o,  v = ((y + 0.5) - cy_o) / fy_o
 *   u2 = u*u, v2 = v*v, r2 = u2 + v2, r4 = r2*r2, r6 = r4*r2, uv = u*v          (du, dv) by model:
 *     0 SIMPLE_PINHOLE (f cx cy), 1 PINHOLE (fx fy cx cy):  du = dv = 0
 *     2 SIMPLE_RADIAL (f cx cy k):            radial = k*r2;            du = u*radial
 *     3 RADIAL (f cx cy k1 k2):               radial = k1*r2 + k2*r4;   du = u*radial
 *     4 OPENCV (fx fy cx cy k1 k2 p1 p2):     radial as RADIAL;  du = (u*radial + (2*p1)*uv) + p2*(r2 + 2*u2)
 *                                                                dv = (v*radial + (2*p2)*uv) + p1*(r2 + 2*v2)
 *     6 FULL_OPENCV (.. k1 k2 p1 p2 k3 k4 k5 k6):  radial = (((1 + k1*r2) + k2*r4) + k3*r6) / (((1 + k4*r2) + k5*r4) + k6*r6);
 *                                                  du = OPENCV's expression - u
 *     8 SIMPLE_RADIAL_FISHEYE (f cx cy k), 9 RADIAL_FISHEYE (f cx cy k1 k2), 5 OPENCV_FISHEYE (fx fy cx cy k1 k2 k3 k4):
 *       r = sqrt(r2); r > 2^-52:  t = atan(r), t2 = t*t, t4 = t2*t2, t6 = t4*t2, t8 = t4*t4,
 *       td = t * (1 + k*t2) | t * ((1 + k1*t2) + k2*t4) | t * ((((1 + k1*t2) + k2*t4) + k3*t6) + k4*t8),
 *       du = (u*td)/r - u;  otherwise du = dv = 0            (dv: v in u's place throughout)
 *   sx = (fx*(u + du) + cx) - 0.5,  sy = (fy*(v + dv) + cy) - 0.5               (f for fx and fy in the one-focal models)
 *   filled = sx >= 0 && sx <= Ws - 1 && sy >= 0 && sy <= Hs - 1   (NaN and +-Inf fail); not filled: the pixel is (0, 0, 0) and no
 *   index is formed.  Filled: x0 = floor(sx), x1 = min(x0 + 1, Ws - 1), wx = sx - x0, rows likewise, and per channel
 *   value = (1 - wy) * ((1 - wx)*p[y0][x0] + wx*p[y0][x1]) + wy * ((1 - wx)*p[y1][x0] + wx*p[y1][x1]),
 *   out = min(max(floor(value + 0.5), 0), 255).
 * Before the launch: ITERMVS_ERR_NULL (src, out or params NULL), ITERMVS_ERR_MODEL (7 FOV, 10 THIN_PRISM_FISHEYE, unknown id),
 * ITERMVS_ERR_DIMS (a size < 1, n_params not the model's count, more than 2^31 - 1 workgroups).
 * ------------------------------------------------------------------------------------------ */
int itermvs_undistort_rgb8(const uint8_t* src, int32_t Hs, int32_t Ws, int32_t model, const double* params, int32_t n_params,
                           double fx_o, double fy_o, double cx_o, double cy_o, int32_t Ho, int32_t Wo, uint8_t* out, double* map,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * Training input side (csrc/train_input.hip).
 *
 * itermvs_image_pyramid_jitter -- datasets/dtu_yao.py:64-77 and datasets/blendedmvs.py:85-101 (read_img in train mode):
 * transforms.ColorJitter(brightness=0.5, contrast=0.5) on the PIL image, then itermvs_image_pyramid's arithmetic.  The
 * jitter is Pillow's (PIL/ImageEnhance.py Brightness / Contrast -> Image.blend(degenerate, image, (float)f)):
 *   blend(a, b, f) = (uint8)(a + f * (b - a)), float32, clipped to 0..255 when f > 1;
 *   brightness: a = 0;  contrast: a = int(mean(L) + 0.5) with L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 over the image
 *   as it stands when contrast is applied.
 * jitter [V] (device): one draw per view; enabled = 0 leaves the view's bytes as they are (level 0 then equals
 *   itermvs_image_pyramid's).  lsum [V] (device uint64 scratch): zeroed and filled here with the per-view sum of L.
 * Outputs as itermvs_image_pyramid (level1..3 may be NULL; H and W multiples of 8 when requested).  Two kernels and a memset.
 * ------------------------------------------------------------------------------------------ */
typedef struct itermvs_jitter {
    float brightness;            /* brightness factor (torchvision's draw, a float32 value) */
    float contrast;              /* contrast factor */
    int32_t contrast_first;      /* 1: contrast is applied before brightness (randperm puts index 1 ahead of index 0) */
    int32_t enabled;             /* 0: no jitter (val mode) */
} itermvs_jitter;

int itermvs_image_pyramid_jitter(const uint8_t* src, int32_t V, int32_t Hs, int32_t Ws, int32_t H, int32_t W,
                                 const itermvs_jitter* jitter, uint64_t* lsum, float* level0, float* level1, float* level2,
                                 float* level3, void* stream);

/* ------------------------------------------------------------------------------------------
 * itermvs_gt_pyramid -- the reference view's ground truth at the four levels, one launch for a batch of B samples:
 *   ITERMVS_GT_DTU        datasets/dtu_yao.py:80-119: depth = raw * p0; cv2.resize(x1/2, NEAREST), centre crop to (W, H),
 *                         level l = cv2.resize(crop, (W >> l, H >> l), NEAREST); mask = (depth_visual > 10) under the same map
 *   ITERMVS_GT_BLENDEDMVS datasets/blendedmvs.py:62-83: depth = (raw * p0) * p1, resized NEAREST to (W, H), then to each level;
 *                         mask = (depth >= p2) & (depth <= p3) at the FILE size, resized NEAREST straight to each level size
 * NEAREST = cv2's map min(floor(d * (1.0 / ((double)dst / src))), src - 1) per axis.
 * depth_rows [B,Hs,Ws] float32: the PFM payload as stored (rows bottom-up; the flip of data_io.py:38 is in the map).
 * mask_src [B,Hs,Ws] uint8: depth_visual (DTU; unused for BlendedMVS).  params [B,4] float32 (device): p0..p3 above.
 * depth_l / mask_l [B,1,H>>l,W>>l] float32, each may be NULL (skipped).  ITERMVS_ERR_DIMS: H or W not a multiple of 8, B < 1,
 * DTU crop outside the x1/2 image, unknown recipe.
 * ------------------------------------------------------------------------------------------ */
#define ITERMVS_GT_DTU 0
#define ITERMVS_GT_BLENDEDMVS 1
int itermvs_gt_pyramid(const float* depth_rows, const uint8_t* mask_src, const float* params, int32_t B, int32_t Hs, int32_t Ws,
                       int32_t H, int32_t W, int32_t recipe, float* depth0, float* depth1, float* depth2, float* depth3,
                       float* mask0, float* mask1, float* mask2, float* mask3, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-mode BatchNorm (+ ReLU) of FeatureNet's ConvBnReLU / ConvBn layers (models/module.py:33-50 under
 * train.py:194-243; torch.nn.BatchNorm2d in train() mode): x, y, dy, dx are dense NCHW fp32 [N,C,H*W].
 *   forward : batch mean / biased variance per channel -> y = [relu]((x - mean) / sqrt(var + eps) * gamma + beta);
 *             save_mean, save_invstd [C] are written for the backward; running_mean / running_var (may be NULL) are
 *             updated in place with `momentum` (running_var with the unbiased variance, like torch).
 *   backward: dx, dgamma, dbeta from dy (the gradient w.r.t. y; the ReLU mask is recomputed from x).
 * `workspace`: itermvs_bn_workspace_floats(N, C, HW) floats of scratch (partials; same size for both directions).
 * ------------------------------------------------------------------------------------------ */
int itermvs_bn_workspace_floats(int32_t N, int32_t C, int32_t HW);
int itermvs_bn_train_forward(const float* x, float* y, int32_t N, int32_t C, int32_t HW, const float* gamma, const float* beta,
                             float eps, float momentum, int32_t relu, float* running_mean, float* running_var,
                             float* save_mean, float* save_invstd, float* workspace, void* stream);
int itermvs_bn_train_backward(const float* x, const float* dy, float* dx, int32_t N, int32_t C, int32_t HW, const float* gamma,
                              const float* beta, const float* save_mean, const float* save_invstd, int32_t relu,
                              float* dgamma, float* dbeta, float* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optional per-launch timing (HIP events recorded on the launch stream around the kernels of
 * itermvs_corr_iter / itermvs_corr_init).  Used by bench.py for the roofline figure.
 * itermvs_profile_enable(n) allocates n event pairs (n = 0 disables and frees);
 * itermvs_profile_collect synchronises the events and returns the number of samples copied:
 * kind[i] (1 = corr_iter, 2 = corr_init) and ms[i].
 * ------------------------------------------------------------------------------------------ */
int itermvs_profile_enable(int32_t capacity);
/* which launches are timed: bit 0 = corr_iter (kind 1), bit 1 = corr_init (kind 2), bit 2 = itermvs_conv2d
 * (kind 3).  Default 0x3. */
int itermvs_profile_set_mask(int32_t mask);
int itermvs_profile_collect(int32_t* kind, float* ms, int32_t max_samples);
/* Launches captured into a hipGraph while profiling is enabled are bracketed by external event-record nodes:
 * itermvs_profile_graph_count() = number of such pairs so far (capture order);
 * itermvs_profile_graph_read(first, count, kind, ms) waits for pairs [first, first+count) of the LATEST replay of
 * their graph and returns how many were read. */
int itermvs_profile_graph_count(void);
int itermvs_profile_graph_read(int32_t first, int32_t count, int32_t* kind, float* ms);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* ITERMVS_HIP_H */
