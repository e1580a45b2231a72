// agt_pnp.hip -- stand-alone cv::solvePnP(SOLVEPNP_ITERATIVE) / cv::projectPoints launches
// (solver body and design notes: agt_pnp_body.h).
#include "agt_pnp_body.h"
#include "agt_pyramid2_body.h"

namespace {

using agt_pnp::load_cam;

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
// Clip submission of the serial step (agt_api_tracker.hip step_serial): the two-level pyramid pass of the NEXT frame rides in this launch
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
        const int st = t / n_pyr, tile = t - st * n_pyr;
        const int by = tile / Y0.gx, bx = tile - by * Y0.gx;
        agt_pyr2::pyr_down2_body(Y0, Y1, bx, by, Y0.src + (long)st * Y0.sbatch, Y0.dst + (long)st * Y0.dbatch, Y1.dst + (long)st * Y1.dbatch, tile_lds);
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

// cv::projectPoints for point i of stream b
template <typename T>
__device__ __forceinline__ void project_one(const AgtProjParams& P, int b, int i)
{
    AgtCamera cam;
    load_cam<T>(P.cam, cam);
    double param[6];
#pragma unroll
    for (int k = 0; k < 6; k++) param[k] = P.pose[(long)b * 6 + k];
    const T* obj = reinterpret_cast<const T*>(P.obj) + (long)b * P.obj_bstride;
    T* out = reinterpret_cast<T*>(P.img_out) + (long)b * P.n * 2;
    double R[9], G[9], u, v, jr[6], jt[6];
    const double X = (double)obj[i * 3], Y = (double)obj[i * 3 + 1], Z = (double)obj[i * 3 + 2];
    if (P.jac) {
        agt_rodrigues<true>(param, R, G);
        agt_project<true>(cam, R, G, param + 3, X, Y, Z, u, v, jr, jt);
        double* J = P.jac + ((long)b * P.n + i) * 12;
#pragma unroll
        for (int k = 0; k < 3; k++) { J[k] = jr[k]; J[3 + k] = jt[k]; J[6 + k] = jr[3 + k]; J[9 + k] = jt[3 + k]; }
    } else {
        agt_rodrigues<false>(param, R, G);
        agt_project<false>(cam, R, G, param + 3, X, Y, Z, u, v, nullptr, nullptr);
    }
    out[i * 2] = (T)u; out[i * 2 + 1] = (T)v;
}

// agt_tag_visibility: the visibility rule (agt_device.h agt_tag_visible) for tag i of stream b
template <typename T>
__device__ __forceinline__ void visible_one(const AgtProjParams& P, int b, int i)
{
    double param[6], R[9], G[9], cs;
#pragma unroll
    for (int k = 0; k < 6; k++) param[k] = P.pose[(long)b * 6 + k];
    agt_rodrigues<false>(param, R, G);
    const T* obj = reinterpret_cast<const T*>(P.obj) + (long)b * P.obj_bstride + (long)i * P.vis_cpt * 3;
    const bool vis = agt_tag_visible(obj, P.vis_cpt, R, param + 3, (double)P.vis_facing, P.vis_cos_max, cs);
    const long o = (long)b * (P.n / P.vis_cpt) + i;
    P.vis_out[o] = vis ? 1 : 0;
    if (P.vis_cos) P.vis_cos[o] = cs;
}

// agt_solve_pnp_consensus: vote and selection for stream b by ONE workgroup of VOTE_WAVES waves (the rule: include/agt_hip.h).  Thread i
// owns corner i and walks the T hypotheses; per hypothesis each wave files its inlier ballot and the sum of its inliers' squared
// residuals in LDS.  Behind one barrier lane t of wave 0 totals hypothesis t (waves in order: the sums are reproducible), thread 0
// elects, and behind a second barrier every thread reads its own bit of the winner's ballots.
constexpr int VOTE_WAVES = 4, VOTE_TAGS = 64;
struct VoteShared {
    unsigned long long ballot[VOTE_WAVES][VOTE_TAGS];
    double ssq[VOTE_WAVES][VOTE_TAGS];
    double tssq[VOTE_TAGS];
    int count[VOTE_TAGS];          // -1: no accepted hypothesis
    int broken[VOTE_TAGS];         // != 0: a corner of the tag is not usable -- the tag is no candidate
    int winner;
};

template <typename T>
__device__ __forceinline__ void vote_stream(const AgtProjParams& P, int b, VoteShared& sh)
{
    const int n = P.n, cpt = P.vote_cpt, nt = n / cpt;
    const int i = (int)threadIdx.x, lane = i & (AGT_WAVE - 1), wave = agt_uniform(i >> 6);
    AgtCamera cam;
    load_cam<T>(P.cam, cam);
    const T* obj = reinterpret_cast<const T*>(P.obj) + (long)b * P.obj_bstride;
    const T* img = reinterpret_cast<const T*>(P.vote_img) + (long)b * n * 2;
    const bool usable = i < n && (!P.vote_mask || P.vote_mask[(long)b * n + i] != 0);
    double X = 0.0, Y = 0.0, Z = 0.0, mx = 0.0, my = 0.0;
    if (i < n) {
        X = (double)obj[i * 3]; Y = (double)obj[i * 3 + 1]; Z = (double)obj[i * 3 + 2];
        mx = (double)img[i * 2]; my = (double)img[i * 2 + 1];
    }
    if (i < VOTE_TAGS) sh.broken[i] = 0;
    __syncthreads();
    if (i < n && !usable) sh.broken[i / cpt] = 1;           // (every writer stores the same value)
    __syncthreads();
    for (int t = 0; t < nt; t++) {
        // accepted: a candidate tag whose solve reported neither SINGULAR nor TOO_FEW and left six finite numbers (uniform)
        const long g = (long)b * nt + t;
        double prm[6];
        bool ok = sh.broken[t] == 0 && (P.vote_info[g * 4 + AGT_INFO_FLAGS] & (AGT_PNP_SINGULAR | AGT_PNP_TOO_FEW)) == 0;
#pragma unroll
        for (int k = 0; k < 6; k++) { prm[k] = P.vote_pose[g * 6 + k]; ok = ok && fabs(prm[k]) <= 1.7976931348623157e308; }     // (false for NaN, inf)
        unsigned long long bal = 0;
        double s = 0.0;
        if (ok) {
            double R[9], G[9], u, v;
            agt_rodrigues<false>(prm, R, G);
            agt_project<false>(cam, R, G, prm + 3, X, Y, Z, u, v, nullptr, nullptr);
            const double zc = R[6] * X + R[7] * Y + R[8] * Z + prm[5];
            const double du = u - mx, dv = v - my, d2 = du * du + dv * dv;
            const bool inl = usable && zc > 0.0 && d2 < P.vote_tau2;          // (false for NaN)
            bal = __ballot(inl);
            s = agt_pnp::wave_sum_f64(inl ? d2 : 0.0);
        }
        if (lane == 0) { sh.ballot[wave][t] = bal; sh.ssq[wave][t] = s; }
        if (i == 0) sh.count[t] = ok ? 0 : -1;
    }
    __syncthreads();
    if (i < nt && sh.count[i] == 0) {
        int cnt = 0;
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < VOTE_WAVES; w++) { cnt += __popcll(sh.ballot[w][i]); s += sh.ssq[w][i]; }
        sh.count[i] = cnt; sh.tssq[i] = s;
    }
    __syncthreads();
    if (i == 0) {
        // most inliers; then the smaller sum of squares; then the lower tag (ascending walk, strict comparisons)
        int best = -1, bc = -1, n_cand = 0, n_hyp = 0;
        double bs = 0.0;
        for (int t = 0; t < nt; t++) {
            if (!sh.broken[t]) n_cand++;
            const int ct = sh.count[t];
            if (ct < 0) continue;
            n_hyp++;
            const double st = sh.tssq[t];
            if (best < 0 || ct > bc || (ct == bc && st < bs)) { best = t; bc = ct; bs = st; }
        }
        if (best >= 0 && bc < P.vote_min) best = -1;
        sh.winner = best;
        if (P.vote_votes) {
            int32_t* vo = P.vote_votes + (long)b * 4;
            vo[0] = best; vo[1] = best >= 0 ? bc : 0; vo[2] = n_cand; vo[3] = n_hyp;
        }
        if (best >= 0) {
            for (int k = 0; k < 6; k++) P.vote_win[(long)b * 6 + k] = P.vote_pose[((long)b * nt + best) * 6 + k];
        }
    }
    __syncthreads();
    const int win = sh.winner;
    if (i < n) P.vote_inl[(long)b * n + i] = win >= 0 ? (uint8_t)((sh.ballot[wave][win] >> lane) & 1) : (uint8_t)0;
}

template <typename T>
__global__ __launch_bounds__(256) void project_kernel(const AgtProjParams P)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (P.vote_inl) {
        __shared__ VoteShared vsh;
        vote_stream<T>(P, b, vsh);           // (vote mode: one workgroup per stream, blockDim.x = 64 * VOTE_WAVES, nothing is written to img_out)
    } else if (P.vis_out) {
        if (i < P.n / P.vis_cpt) visible_one<T>(P, b, i);      // (visibility mode: one thread per tag, nothing is projected)
    } else if (i < P.n) project_one<T>(P, b, i);
    if (P.host_seq) {
        // one-block launch of agt_project_points_host: every wave's outputs (host-mapped memory) are performed at system scope before the
        // barrier, then one lane tells the polling host thread
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        __syncthreads();
        if (threadIdx.x < AGT_WAVE) agt_host_seq_store(P.host_seq, P.host_seq_base, threadIdx.x == 0);
    }
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

hipError_t agt_launch_project(hipStream_t stream, const AgtProjParams& p, int B)
{
    if (p.vote_inl && (p.n > 64 * VOTE_WAVES || p.vote_cpt <= 0 || p.n / p.vote_cpt > VOTE_TAGS)) return hipErrorInvalidValue;
    const int items = p.vote_inl ? 1 : p.vis_out ? p.n / p.vis_cpt : p.n;         // (vote mode: one workgroup per stream; visibility mode: tags)
    dim3 grid((items + 255) / 256, B), block(256);
    if (p.dtype == AGT_F64) hipLaunchKernelGGL(project_kernel<double>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(project_kernel<float>, grid, block, 0, stream, p);
    return hipGetLastError();
}
