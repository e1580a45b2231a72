// agt_pyramid.hip -- stand-alone cv::pyrDown launch (body: agt_pyramid_body.h).
// Replaces the pyramid build inside cv.calcOpticalFlowPyrLK (north-star step).
// Algorithmic bytes per launch: sw*sh read + dw*dh written (per image).
#include "agt_knobs.h"
#include "agt_pyramid2_body.h"
#include "agt_pyramid3_body.h"
#include "agt_pyramid4_body.h"

namespace {

__global__ __launch_bounds__(agt_pyr::NT) void pyr_down_kernel(const AgtPyrArgs A)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    // XCD-aware tile order (agt_kernels.h agt_xcd_order): workgroups are dealt round-robin to the X XCDs (each with its own L2), so
    // workgroup b takes tile (b % X) * per_xcd + b / X -- every XCD walks a CONTIGUOUS row-major run of
    // tiles and the 128-B lines shared by neighbouring tiles (16-B side halos, 3 halo rows) hit in its L2
    // instead of being fetched once per XCD.
    const int t = agt_xcd_order((int)blockIdx.x, (int)gridDim.x, A.xshift);
    const int per_img = A.gx * A.gy;
    if (t >= per_img * A.B) return;
    const int bz = t / per_img, r = t - bz * per_img;
    const int by = r / A.gx;
    agt_pyr::pyr_down_body(A, r - by * A.gx, by, A.src + (long)bz * A.sbatch, A.dst + (long)bz * A.dbatch, lds);
}

// register-rolling form (agt_pyramid3_body.h): A.gx = workgroups per image, A.strip_rows = output rows per strip; same XCD-aware order
__global__ __launch_bounds__(agt_pyr::NT) void pyr_roll_kernel(const AgtPyrArgs A)
{
    const int t = agt_xcd_order((int)blockIdx.x, (int)gridDim.x, A.xshift);
    if (t >= A.gx * A.B) return;
    const int bz = t / A.gx;
    agt_pyr3::pyr_roll_body(A, t - bz * A.gx, A.src + (long)bz * A.sbatch, A.dst + (long)bz * A.dbatch);
}

// two levels per pass (agt_pyramid2_body.h): same XCD-aware tile order, tiles of 64 x 16 L2 pixels
__global__ __launch_bounds__(agt_pyr::NT) void pyr_down2_kernel(const AgtPyrArgs A0, const AgtPyrArgs A1)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int t = agt_xcd_order((int)blockIdx.x, (int)gridDim.x, A0.xshift);
    const int per_img = A0.gx * A0.gy;
    if (t >= per_img * A0.B) return;
    const int bz = t / per_img;
    agt_pyr2::pyr2_tile_of_stream(A0, A1, bz, t - bz * per_img, lds);
}

// Fused upload (agt_track_host_frame): ONE gray frame read from pinned host memory (A0.src: its device address), level 0 copied to
// HBM (`copy`), levels 1 and 2 written -- the two-level register-rolling pass with COPY (agt_pyramid4_body.h)
__global__ __launch_bounds__(agt_pyr::NT) void pyr_upload2_kernel(const AgtPyrArgs A0, const AgtPyrArgs A1, uint8_t* copy, const int cpitch)
{
    const int t = agt_xcd_order((int)blockIdx.x, (int)gridDim.x, A0.xshift);
    if (t >= A0.gx) return;
    agt_pyr4::pyr_roll2_body<true, false>(A0, A1, t, A0.src, A0.dst, A1.dst, copy, cpitch);
}

// two levels per pass, register-rolling form with alternating strip directions (agt_pyramid4_body.h): A0.gx = workgroups per image,
// A0.strip_rows = level-2 rows per strip
__global__ __launch_bounds__(agt_pyr::NT) void pyr_roll2_kernel(const AgtPyrArgs A0, const AgtPyrArgs A1)
{
    const int t = agt_xcd_order((int)blockIdx.x, (int)gridDim.x, A0.xshift);
    if (t >= A0.gx * A0.B) return;
    const int bz = t / A0.gx;
    agt_pyr4::pyr_roll2_body(A0, A1, t - bz * A0.gx, A0.src + (long)bz * A0.sbatch, A0.dst + (long)bz * A0.dbatch, A1.dst + (long)bz * A1.dbatch);
}

}  // namespace

void agt_pyr2_grid(int w2, int h2, int* gx, int* gy)
{
    *gx = (w2 + agt_pyr2::TW2 - 1) / agt_pyr2::TW2;
    *gy = (h2 + agt_pyr2::TH2 - 1) / agt_pyr2::TH2;
}

void agt_pyr_grid(int dw, int dh, int* gx, int* gy)
{
    *gx = (dw + agt_pyr::TW - 1) / agt_pyr::TW;
    *gy = (dh + agt_pyr::TH - 1) / agt_pyr::TH;
}

// one pass's argument block from its source and destination level (the destination's size is implied: (w + 1) / 2) and B images:
// tiled form, the grid left to the planner
static void pyr_args(const AgtLevel& src, const AgtLevel& dst, int B, AgtPyrArgs& A)
{
    A.src = src.ptr; A.sw = src.w; A.sh = src.h; A.spitch = src.pitch; A.sbatch = src.bstride;
    A.dst = const_cast<uint8_t*>(dst.ptr); A.dw = (src.w + 1) / 2; A.dh = (src.h + 1) / 2; A.dpitch = dst.pitch; A.dbatch = dst.bstride;
    A.B = B; A.strip_rows = 0;
    A.xshift = agt_chip_current().xshift; A.topdown = 0;
}

// "The register-rolling form can take this source and destination": 16-byte loads of whole groups, at least two of them per row,
// 8-byte stores of level 1, buffer descriptors (32-bit sizes and offsets) over source and destination.  A: the pass (of a two-level
// pass: its level 0 -> 1 block); src_align / dst_align: OR of every source / destination address of the launch.  What differs:
//   min_h       8 for one level, 32 for two (neither figure has a measurement or a derivation on record: profiles/pyr_refactor.md)
//   dst2_align  two levels: OR of the level-2 addresses, pitch and stride; 4 bytes -- a lane stores 4 level-2 pixels
//   copy_align, cpitch  fused upload: level 0 is copied with 16-byte stores through a descriptor of sh * cpitch bytes
static bool pyr_roll_ok(const AgtPyrArgs& A, uintptr_t src_align, uintptr_t dst_align, int min_h, uintptr_t dst2_align = 0,
                        uintptr_t copy_align = 0, long cpitch = 0)
{
    return ((src_align | (uintptr_t)A.spitch | (uintptr_t)A.sbatch | (uintptr_t)A.sw | copy_align | (uintptr_t)cpitch) & 15) == 0 &&
           ((dst_align | (uintptr_t)A.dpitch | (uintptr_t)A.dbatch) & 7) == 0 && (dst2_align & 3) == 0 &&
           A.sw >= 32 && A.sh >= min_h && (long)A.sh * A.spitch < (1L << 31) && (long)A.sh * cpitch < (1L << 31) && (long)A.dh * A.dpitch < (1L << 31);
}

// the two-level pass in A[0], A[1] runs register-rolling with strips of `oh` level-2 rows (gx = workgroups per image, gy = 1), or
// tiled (oh = 0: the tile grid of the pass); said in both blocks
static void pyr2_set_form(AgtPyrArgs* A, int oh)
{
    if (oh) { A[0].gx = agt_pyr4::roll2_blocks(A[0].sw, A[1].dh, oh); A[0].gy = 1; }
    else agt_pyr2_grid(A[1].dw, A[1].dh, &A[0].gx, &A[0].gy);
    A[0].strip_rows = A[1].strip_rows = oh; A[1].gx = A[0].gx; A[1].gy = A[0].gy;
}

void agt_pyr2_args(const AgtLevel* lv, int B, AgtPyrArgs* A)
{
    for (int k = 0; k < 2; k++) pyr_args(lv[k], lv[k + 1], B, A[k]);
    pyr2_set_form(A, 0);
}

// The register-rolling form of the two-level pass where it applies: strip_rows = level-2 rows per strip, gx = workgroups per image,
// gy = 1 (in both blocks); else the tiled form as agt_pyr2_args sets it up (strip_rows = 0).  src_align / dst_align: OR of every
// source / destination address of the launch (both destination levels); frames: images per stream in the launch.
void agt_pyr2_plan(AgtPyrArgs* A, uintptr_t src_align, uintptr_t dst_align, int frames, int oh_cap)
{
    AgtPyrArgs& A0 = A[0]; AgtPyrArgs& A1 = A[1];
    pyr2_set_form(A, 0);
    const bool ok = pyr_roll_ok(A0, src_align, dst_align, 32, dst_align | (uintptr_t)A1.dpitch | (uintptr_t)A1.dbatch);
    // Round 4 measured this pass and did not ship it: every strip walked top-down, its 9 halo rows came from memory a second time
    // ((4 oh2 + 9) / (4 oh2) of the image: FETCH_SIZE 76.1 MB for 59.0 MB of frames at oh2 = 8) and a lane spent ~70 VALU per level-0
    // row; 64 x 720p: 24.0-25.5 us per pass against 24.9 for two single-level passes.  Round 5 ships it for launches of >= 16 images:
    // alternating strip directions (neighbouring strips read their shared rows at the same time: FETCH_SIZE 60.4 MB) and the lean
    // horizontal / vertical passes (agt_pyramid_body.h hgroup8b / vgroup8b: ~50 VALU per row).  The pipelined cold-pair step of
    // BASELINE configs[2] (which is VALU- and HBM-bound together): 54.6-56.2 -> 48.1-49.1 us; traffic of the pass 94.5 -> 78.9 MB
    // against the 77.4 MB of SURVEY 8d (profiles/r05_experiments.md).  Smaller launches keep the tiled pass (one frame: 6.5-7.3 us
    // tiled, 5.9-8.5 rolling).
    const long images = (long)A0.B * (frames > 0 ? frames : 1);
    int want = images >= 16 ? 1 : 0;
    // knobs: AGT_PYR4=0 / 1 forces the choice, AGT_PYR4_OH=n the strip height, AGT_PYR4_REV=0 top-down strips only
    { const long on = AGT_KNOB("AGT_PYR4", -1); if (on >= 0) want = (int)on; }
    A0.topdown = A1.topdown = AGT_KNOB("AGT_PYR4_REV", 1) ? 0 : 1;
    if (!ok || !want) return;
    // strip height (level-2 rows, even): ~2 waves on each SIMD where the launch has that many units (the pass shares the chip with
    // the LK kernels of other batches; measured on 64 x 720p inside the pipelined step: oh2 = 4: 53.5 us, 6: 50.3, 8: 48.8-49.1,
    // 10: 48.1, 12: 49.7, 16: 52.8), strips of at most 16 rows (73 level-0 rows: 14 % of them the halo), at least 2 (17 rows)
    const int ncol = ((A0.sw >> 4) + agt_pyr4::TILE_GROUPS - 1) / agt_pyr4::TILE_GROUPS;
    const long want_units = 32L * agt_chip_current().cus;                 // 2 waves x 4 units x 4 SIMDs per CU
    long per_image = (want_units + images - 1) / images;
    long strips = (per_image + ncol - 1) / ncol;
    if (strips < 1) strips = 1;
    constexpr int Q = agt_pyr4::L2_PER_TRIP;
    int oh = (int)((A1.dh + strips - 1) / strips + Q - 1) / Q * Q;
    // oh_cap (round 6): 16 for a launch of its own (agt_pyramid_build, agt_pyramid_build_pair: the pass IS the step's long pole there and
    // every strip pays 9 halo rows of loads and arithmetic); AGT_SPLIT_PYR_OH = 6 (agt_tracker_frames.hip) for the pyramid role of the split pipeline,
    // whose launch of up to 1,024 images runs for hundreds of microseconds BESIDE the per-frame LK launches: 64 streams x 16 frames, us per
    // step over four boxes 16: 36.7-37.6, 10: 36.0-36.2, 8: 35.7-36.3, 6: 35.1-35.9, 4: 35.4-36.3, 2: 40.6 (profiles/r06_experiments.md 17)
    // -- short-lived pyramid waves give their slots back sooner
    if (oh_cap < Q) oh_cap = Q;
    oh = oh < Q ? Q : (oh > oh_cap ? oh_cap : oh);
    { const long f = AGT_KNOB("AGT_PYR4_OH", 0); if (f > 0) oh = (int)(f + Q - 1) / Q * Q; }
    pyr2_set_form(A, oh);
}

// Fused upload + two-level pyramid of ONE frame: src = device address of the caller's gray frame in pinned host memory; copy = the
// frame's level 0 in HBM.  hipErrorInvalidValue when the geometry does not fit the rolling form (the caller then copies and builds).
hipError_t agt_launch_pyr_upload2(hipStream_t stream, const uint8_t* src, int sw, int sh, long spitch, uint8_t* copy, long cpitch,
                                  uint8_t* dst1, long dpitch1, uint8_t* dst2, long dpitch2)
{
    const int w1 = (sw + 1) / 2, h1 = (sh + 1) / 2;
    const AgtLevel lv[3] = { { src, spitch, 0, sw, sh }, { dst1, dpitch1, 0, w1, h1 }, { dst2, dpitch2, 0, (w1 + 1) / 2, (h1 + 1) / 2 } };
    AgtPyrArgs A[2];
    agt_pyr2_args(lv, 1, A);
    AgtPyrArgs& A0 = A[0]; AgtPyrArgs& A1 = A[1];
    if (!pyr_roll_ok(A0, (uintptr_t)src, (uintptr_t)dst1, 32, (uintptr_t)dst2 | (uintptr_t)dpitch2, (uintptr_t)copy, cpitch)) return hipErrorInvalidValue;
    // two level-2 rows per strip (17 level-0 rows a lane): the most units one frame gives, measured 22.9 us from pinned host memory
    // (4: 24.7, 8: 26.2); the rows a strip reads twice come out of the L2, not over PCIe again
    pyr2_set_form(A, agt_pyr4::L2_PER_TRIP);
    hipLaunchKernelGGL(pyr_upload2_kernel, dim3(agt_xcd_grid(A0.gx, A0.xshift)), dim3(agt_pyr::NT), 0, stream, A0, A1, copy, (int)cpitch);
    return hipGetLastError();
}

// the two-level pass as agt_pyr2_args + agt_pyr2_plan left it in A[0], A[1]: both levels written, one launch
hipError_t agt_launch_pyr_down2(hipStream_t stream, const AgtPyrArgs* A)
{
    const dim3 grid(agt_xcd_grid((long)agt_pyr_blocks(A[0]) * A[0].B, A[0].xshift));
    if (agt_pyr_rolling(A[0])) hipLaunchKernelGGL(pyr_roll2_kernel, grid, dim3(agt_pyr::NT), 0, stream, A[0], A[1]);
    else hipLaunchKernelGGL(pyr_down2_kernel, grid, dim3(agt_pyr::NT), agt_pyr2::PYR2_LDS_BYTES, stream, A[0], A[1]);
    return hipGetLastError();
}

// Geometry of one pyrDown pass for A.src / A.dst (pointers, pitches, sizes and B filled in): the register-rolling form where
// it applies (A.strip_rows = output rows per strip, A.gx = workgroups per image, A.gy = 1), else the tiled form (strip_rows = 0, tile grid).
// `src_align` / `dst_align`: OR of every source / destination address the launch will see (frames of a group, batch strides).
void agt_pyr_plan(AgtPyrArgs* pA, uintptr_t src_align, uintptr_t dst_align, int frames)
{
    AgtPyrArgs& A = *pA;
    A.strip_rows = 0;
    A.xshift = agt_chip_current().xshift; A.topdown = 0;
    agt_pyr_grid(A.dw, A.dh, &A.gx, &A.gy);
    if (!AGT_KNOB("AGT_PYR3", 1)) return;       // (knobs: AGT_PYR3=0 keeps the tiled kernel, AGT_PYR3_OH=n forces the strip height)
    if (!pyr_roll_ok(A, src_align, dst_align, 8)) return;
    // strip height: enough units (four per wave) to put ~3 waves on each of the chip's SIMDs (1024 on MI355X: 12,288 units) -- a wave keeps 8 KB of reads in
    // flight --, strips no longer than 16 output rows (measured on 64 x 720p, L0 -> L1: 8 rows 17.8 us, 16: 17.0, 24: 21.2,
    // 32: 22.1, 48: 27 -- the tiled kernel: 18.6), no shorter than 4 (3 halo rows per strip are re-read through the L2)
    const long images = (long)A.B * (frames > 0 ? frames : 1);
    const int ncol = ((A.sw >> 4) + 15) >> 4;
    const long want_units = 48L * agt_chip_current().cus;                 // 3 waves x 4 units x 4 SIMDs per CU
    long per_image = (want_units + images - 1) / images;
    long strips = (per_image + ncol - 1) / ncol;
    if (strips < 1) strips = 1;
    int oh = (int)(A.dh / strips) & ~3;
    oh = oh < 4 ? 4 : (oh > 16 ? 16 : oh);
    { const long f = AGT_KNOB("AGT_PYR3_OH", 0); if (f > 0) oh = (int)f & ~3; }
    A.strip_rows = oh;
    A.gx = agt_pyr3::roll_blocks(A.sw, A.dh, oh);
    A.gy = 1;
}

hipError_t agt_launch_pyr_down(hipStream_t stream, const AgtLevel& src, const AgtLevel& dst, int B)
{
    AgtPyrArgs A;
    pyr_args(src, dst, B, A);
    agt_pyr_plan(&A, (uintptr_t)A.src, (uintptr_t)A.dst, 1);
    const dim3 grid(agt_xcd_grid((long)agt_pyr_blocks(A) * B, A.xshift));
    if (agt_pyr_rolling(A)) hipLaunchKernelGGL(pyr_roll_kernel, grid, dim3(agt_pyr::NT), 0, stream, A);
    else hipLaunchKernelGGL(pyr_down_kernel, grid, dim3(agt_pyr::NT), agt_pyr::PYR_LDS_BYTES, stream, A);
    return hipGetLastError();
}
