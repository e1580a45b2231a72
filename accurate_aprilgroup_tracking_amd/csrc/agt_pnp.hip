// agt_pnp.hip -- stand-alone cv::solvePnP(SOLVEPNP_ITERATIVE) launches
// (solver body and design notes: agt_pnp_body.h; cv::projectPoints and its kin: agt_project.hip).
#include "agt_pnp_body.h"
#include "agt_pyramid2_body.h"

namespace {

template <typename T, int PPL>
__global__ __launch_bounds__(AGT_WAVE) void pnp_kernel(const AgtPnpParams P)
{
    __shared__ agt_pnp::PnpShared sh;
    // (issue priority 2 / 3 for the solver's wave beside co-tenant trackers at priority 1 gained nothing: profiles/r06_experiments.md)
    agt_pnp::pnp_body<T, PPL, agt_pnp::PnpNoHook, false, 1, false, true, true>(P, blockIdx.x, sh, P.img, P.mask, P.state_out);
    if (P.host_seq && blockIdx.x == 0) agt_host_seq_store(P.host_seq, P.host_seq_base, threadIdx.x == 0);
}

// n > 64: four waves.  A solve that starts from a guess is shared by all of them (agt_pnp_body.h, COOP); one without (first
// frame of a tracker, after a gate rejection, cv2-shaped calls without useExtrinsicGuess) is wave 0's, four points per lane.
constexpr int COOP_WAVES = agt_pnp::MAX_PPL;
// Clip submission of the serial step (agt_tracker_frames.hip step_serial): the two-level pyramid pass of the NEXT frame rides in this launch
// as extra workgroups (blockIdx.x >= n_solve; tile t of stream s at n_solve + s * n_pyr + t) -- the solve is one workgroup per
// stream, the rest of the chip idles beside it, and alone the pass was a 6.5 us launch at the head of the next frame's chain.
template <typename T>
__global__ __launch_bounds__(AGT_WAVE * COOP_WAVES) void pnp_coop_kernel(const AgtPnpParams P, const AgtPyrArgs Y0, const AgtPyrArgs Y1,
                                                                         const int n_solve, const int n_pyr)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t tile_lds[];       // pyramid tiles only (0 bytes without the job)
    __shared__ agt_pnp::PnpShared sh;
    if ((int)blockIdx.x >= n_solve) {
        const int t = (int)blockIdx.x - n_solve;
        const int st = t / n_pyr;
        agt_pyr2::pyr2_tile_of_stream(Y0, Y1, st, t - st * n_pyr, tile_lds);
        return;
    }
    const int b = blockIdx.x;
    const bool guess = P.track ? (agt_uniform(P.track[b].has_guess) && P.enhance_ape) : P.use_guess != 0;
    // every wave has read the decision before wave 0 (alone, in the branch without a guess) may rewrite track[b].has_guess
    __syncthreads();
    if (guess) agt_pnp::pnp_body<T, 1, agt_pnp::PnpNoHook, false, COOP_WAVES, false, true, true>(P, b, sh, P.img, P.mask, P.state_out);
    else if (threadIdx.x < AGT_WAVE) agt_pnp::pnp_body<T, agt_pnp::MAX_PPL, agt_pnp::PnpNoHook, false, 1, false, true, true>(P, b, sh, P.img, P.mask, P.state_out);
    if (P.host_seq && b == 0 && threadIdx.x < AGT_WAVE) agt_host_seq_store(P.host_seq, P.host_seq_base, threadIdx.x == 0);      // (wave 0 writes the record in both bodies)
}

template <typename T>
hipError_t launch_pnp_t(hipStream_t stream, const AgtPnpParams& p, int B, const AgtPyrArgs* ride)
{
    dim3 grid(B), block(AGT_WAVE);
    if (p.n <= AGT_WAVE) {
        if (ride) return hipErrorInvalidValue;                    // (one-wave workgroups cannot carry pyramid tiles: agt_pnp_can_ride)
        hipLaunchKernelGGL((pnp_kernel<T, 1>), grid, block, 0, stream, p);
    } else {
        const AgtPyrArgs none = AgtPyrArgs();
        const int n_pyr = ride ? ride[0].gx * ride[0].gy : 0;
        hipLaunchKernelGGL((pnp_coop_kernel<T>), dim3((unsigned)(B + n_pyr * B)), dim3(AGT_WAVE * COOP_WAVES),
                           ride ? (size_t)agt_pyr2::PYR2_LDS_BYTES : 0, stream, p, ride ? ride[0] : none, ride ? ride[1] : none, B, n_pyr > 0 ? n_pyr : 1);
    }
    return hipGetLastError();
}

}  // namespace

bool agt_pnp_can_ride(int n) { return n > AGT_WAVE && n <= AGT_WAVE * agt_pnp::MAX_PPL; }

hipError_t agt_launch_pnp(hipStream_t stream, const AgtPnpParams& p, int B, const AgtPyrArgs* ride)
{
    if (p.n > AGT_WAVE * agt_pnp::MAX_PPL) return hipErrorInvalidValue;
    return p.dtype == AGT_F64 ? launch_pnp_t<double>(stream, p, B, ride) : launch_pnp_t<float>(stream, p, B, ride);
}
