// agt_project.hip -- the projection family: cv::projectPoints and the four jobs that grew beside it (tag visibility, the consensus
// vote, the motion-predicted flow seeds, the back seeds of the forward-backward check).  One kernel, one argument block and one launcher
// per job (agt_kernels.h); the launcher owns the job's grid shape and limits.
#undef AGT_PNP_STAMPS        // (the diagnostic build's solver stamps belong to agt_pnp.hip)
#include "agt_pnp_body.h"

namespace {

using agt_pnp::load_cam;

// cv::projectPoints for point i of stream b
template <typename T>
__device__ __forceinline__ void project_one(const AgtPointsParams& P, int b, int i)
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
__device__ __forceinline__ void visible_one(const AgtVisibleParams& P, int b, int i)
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
__device__ __forceinline__ void vote_stream(const AgtVoteParams& P, int b, VoteShared& sh)
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

// agt_predict_flow / agt_tracker_predict: the seed rule for stream b by ONE workgroup of FLOW_WAVES waves (the rule: include/agt_hip.h).
// Wave 0 does the pose algebra, which is uniform, once and leaves the two rotations in LDS; behind one barrier thread i projects corner i
// under the newer and the predicted pose; every wave files a ballot of its objections (a usable corner behind the camera, a flow that is
// not finite or beyond the cap) and the largest flow component of its corners; behind a second barrier every thread reads the verdict.
constexpr int FLOW_WAVES = 4;
struct FlowShared {
    double R1[9], t1[3], Rp[9], tp[3];
    unsigned long long objection[FLOW_WAVES];
    float fmax[FLOW_WAVES];
    int state;                     // 0: no prediction (tracker: the two records were not both accepted), 1: predicted, 2: a pose number is not finite
};

template <typename T>
__device__ __forceinline__ void flow_stream(const AgtFlowParams& P, int b, FlowShared& sh)
{
    const int n = P.n;
    const int i = (int)threadIdx.x, lane = i & (AGT_WAVE - 1), wave = agt_uniform(i >> 6);
    double* hist = P.flow_hist ? P.flow_hist + (long)b * AGT_PRED_STRIDE : nullptr;
    if (wave == 0) {
        const double* older = hist ? hist + AGT_PRED_BEFORE : P.flow_older + (long)b * P.flow_pstride;
        const double* newer = hist ? hist + AGT_PRED_LAST : P.flow_newer + (long)b * P.flow_pstride;
        double p2[6], p1[6];
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            p2[k] = older[k]; p1[k] = newer[k];
            finite = finite && fabs(p2[k]) <= 1.7976931348623157e308 && fabs(p1[k]) <= 1.7976931348623157e308;     // (false for NaN, inf)
        }
        int state = finite ? 1 : 2;
        if (hist && !(hist[AGT_PRED_LAST + 6] != 0.0 && hist[AGT_PRED_BEFORE + 6] != 0.0)) state = 0;
        state = agt_uniform(state);
        double pp[6];
#pragma unroll
        for (int k = 0; k < 6; k++) pp[k] = __builtin_nan("");
        if (state == 1) {
            // D = R1 R2^T (the camera-frame motion older -> newer), applied once more: Rp = D R1, tp = D (t1 - t2) + t1
            double R2[9], R1[9], D[9], Rp[9];
            agt_rodrigues<false>(p2, R2, nullptr);
            agt_rodrigues<false>(p1, R1, nullptr);
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) D[r * 3 + c] = R1[r * 3] * R2[c * 3] + R1[r * 3 + 1] * R2[c * 3 + 1] + R1[r * 3 + 2] * R2[c * 3 + 2];
            agt_mat3_mul(D, R1, Rp);
            const double d0 = p1[3] - p2[3], d1 = p1[4] - p2[4], d2 = p1[5] - p2[5];
#pragma unroll
            for (int r = 0; r < 3; r++) pp[3 + r] = D[r * 3] * d0 + D[r * 3 + 1] * d1 + D[r * 3 + 2] * d2 + p1[3 + r];
            agt_rodrigues_inv(Rp, pp);
            agt_rodrigues<false>(pp, Rp, nullptr);          // (the corners are projected under the predicted POSE, as agt_project_points would)
            if (lane < 9) { sh.R1[lane] = R1[lane]; sh.Rp[lane] = Rp[lane]; }
            if (lane < 3) { sh.t1[lane] = p1[3 + lane]; sh.tp[lane] = pp[3 + lane]; }
        }
        if (lane == 0) sh.state = state;
        if (P.flow_pred && lane < 6) P.flow_pred[(long)b * 6 + lane] = pp[lane];
    }
    __syncthreads();
    const int state = sh.state;
    const bool usable = i < n && (!P.flow_mask || P.flow_mask[(long)b * n + i] != 0);
    float fx = 0.f, fy = 0.f, mag = 0.f;
    bool objects = false;
    if (state == 1 && usable) {
        AgtCamera cam;
        load_cam<T>(P.cam, cam);
        const T* obj = reinterpret_cast<const T*>(P.obj) + (long)b * P.obj_bstride;
        const double X = (double)obj[i * 3], Y = (double)obj[i * 3 + 1], Z = (double)obj[i * 3 + 2];
        double R[9], t[3], u1, v1, up, vp;
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = sh.R1[k];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = sh.t1[k];
        agt_project<false>(cam, R, nullptr, t, X, Y, Z, u1, v1, nullptr, nullptr);
        const double z1 = R[6] * X + R[7] * Y + R[8] * Z + t[2];
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = sh.Rp[k];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = sh.tp[k];
        agt_project<false>(cam, R, nullptr, t, X, Y, Z, up, vp, nullptr, nullptr);
        const double zp = R[6] * X + R[7] * Y + R[8] * Z + t[2];
        fx = (float)(up - u1); fy = (float)(vp - v1);
        mag = fmaxf(fabsf(fx), fabsf(fy));
        // (written so that a NaN objects: fmaxf drops one, hence the components are tested themselves)
        objects = !(z1 > 0.0 && zp > 0.0) || !(fabsf(fx) <= 3.4028234663852886e38f && fabsf(fy) <= 3.4028234663852886e38f) || !(mag <= P.flow_cap);
    }
    const unsigned long long bal = __ballot(objects);
    float wmax = objects ? 0.f : mag;
    for (int o = 32; o >= 1; o >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, o));
    if (lane == 0) { sh.objection[wave] = bal; sh.fmax[wave] = wmax; }
    __syncthreads();
    unsigned long long any = 0;
    float fm = 0.f;
#pragma unroll
    for (int w = 0; w < FLOW_WAVES; w++) { any |= sh.objection[w]; fm = fmaxf(fm, sh.fmax[w]); }
    const bool trusted = state == 1 && any == 0;
    if (i < n) {
        const long o = (long)b * n + i;
        const float2 p = reinterpret_cast<const float2*>(P.flow_prev)[o];
        const bool move = trusted && usable;
        if (!move) fx = fy = 0.f;
        reinterpret_cast<float2*>(P.flow_seed)[o] = move ? make_float2(p.x + fx, p.y + fy) : p;
        if (P.flow_out) reinterpret_cast<float2*>(P.flow_out)[o] = make_float2(fx, fy);
    }
    if (i == 0) {
        const float verdict = state == 0 ? 0.f : trusted ? fm : -1.f;
        if (P.flow_max) P.flow_max[b] = verdict;
        if (hist) {
            // the frame's pose step files its record in `last`; until it does, `last` says "not accepted"
#pragma unroll
            for (int k = 0; k < 7; k++) hist[AGT_PRED_BEFORE + k] = hist[AGT_PRED_LAST + k];
            hist[AGT_PRED_LAST + 6] = 0.0;
            hist[AGT_PRED_FLOW] = (double)verdict;
        }
    }
}

// backward seeds of the tracker's forward-backward check under agt_tracker_predict: arrival - flow, float32
__device__ __forceinline__ void flow_back_one(const AgtFlowBackParams& P, int b, int i)
{
    const long o = (long)b * P.n + i;
    const float2 q = reinterpret_cast<const float2*>(P.flow_prev)[o], f = reinterpret_cast<const float2*>(P.flow_out)[o];
    reinterpret_cast<float2*>(P.flow_back)[o] = make_float2(q.x - f.x, q.y - f.y);
}

template <typename T>
__global__ __launch_bounds__(256) void project_points_kernel(const AgtPointsParams P)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P.n) project_one<T>(P, blockIdx.y, i);
    if (P.host_seq) {
        // one-block launch of agt_project_points_host: every wave's outputs (host-mapped memory) are performed at system scope before the
        // barrier, then one lane tells the polling host thread
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        __syncthreads();
        if (threadIdx.x < AGT_WAVE) agt_host_seq_store(P.host_seq, P.host_seq_base, threadIdx.x == 0);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void visible_kernel(const AgtVisibleParams P)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P.n / P.vis_cpt) visible_one<T>(P, blockIdx.y, i);
}

template <typename T>
__global__ __launch_bounds__(AGT_WAVE * VOTE_WAVES) void vote_kernel(const AgtVoteParams P)
{
    __shared__ VoteShared sh;
    vote_stream<T>(P, blockIdx.y, sh);
}

template <typename T>
__global__ __launch_bounds__(AGT_WAVE * FLOW_WAVES) void flow_kernel(const AgtFlowParams P)
{
    __shared__ FlowShared sh;
    flow_stream<T>(P, blockIdx.y, sh);
}

__global__ __launch_bounds__(256) void flow_back_kernel(const AgtFlowBackParams P)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P.n) flow_back_one(P, blockIdx.y, i);
}

// <<<grid, 256>>> of the f32 or the f64 instance of a typed kernel
template <class P>
hipError_t launch_typed(void (*f32)(P), void (*f64)(P), dim3 grid, hipStream_t stream, const P& p)
{
    hipLaunchKernelGGL(p.dtype == AGT_F64 ? f64 : f32, grid, dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace

hipError_t agt_launch_points(hipStream_t stream, const AgtPointsParams& p, int B)
{
    return launch_typed(project_points_kernel<float>, project_points_kernel<double>, dim3((p.n + 255) / 256, B), stream, p);
}

hipError_t agt_launch_visible(hipStream_t stream, const AgtVisibleParams& p, int B)
{
    return launch_typed(visible_kernel<float>, visible_kernel<double>, dim3((p.n / p.vis_cpt + 255) / 256, B), stream, p);
}

hipError_t agt_launch_vote(hipStream_t stream, const AgtVoteParams& p, int B)
{
    if (p.n > AGT_WAVE * VOTE_WAVES || p.vote_cpt <= 0 || p.n / p.vote_cpt > VOTE_TAGS) return hipErrorInvalidValue;
    return launch_typed(vote_kernel<float>, vote_kernel<double>, dim3(1, B), stream, p);
}

hipError_t agt_launch_flow(hipStream_t stream, const AgtFlowParams& p, int B)
{
    if (p.n > AGT_WAVE * FLOW_WAVES || (p.n > 0 && !p.flow_seed)) return hipErrorInvalidValue;
    return launch_typed(flow_kernel<float>, flow_kernel<double>, dim3(1, B), stream, p);
}

hipError_t agt_launch_flow_back(hipStream_t stream, const AgtFlowBackParams& p, int B)
{
    hipLaunchKernelGGL(flow_back_kernel, dim3((p.n + 255) / 256, B), dim3(256), 0, stream, p);
    return hipGetLastError();
}
