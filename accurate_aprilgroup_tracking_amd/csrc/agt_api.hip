// agt_api.hip -- C ABI (include/agt_hip.h) over the gfx950 kernels: error strings, context lifecycle, the device table and the
// library's stream pool.  The calls live in agt_api_calls.hip, the tracker in agt_api_tracker.hip (its launch forms:
// agt_tracker_frames.hip), undistortion in agt_api_undistort.hip.
#include "agt_ctx.h"
#include "agt_side_math.h"
#include <new>
#include <string.h>
#include <math.h>
#include <atomic>
#include <mutex>
#include <vector>

namespace {

int g_last_hip = 0;      // last failing HIP call made without a context (agt_create)

// matTilt | invMatTilt of a coefficient vector (the arithmetic: agt_side_math.h), the identity unless it is tilted: 14 coefficients =
// the 12 + the tilted-sensor angles (tau_x, tau_y), which cv2.calibrateCamera returns non-zero only under CALIB_TILTED_MODEL -- the
// reference calibrates 5 coefficients, calibrate_camera.py:178
void tilt_matrices(const double* dist, int ndist, AgtTiltHost* t)
{
    static const double I3[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
    memcpy(t->m, I3, sizeof(I3)); memcpy(t->m + 9, I3, sizeof(I3));
    t->on = 0;
    if (ndist != 14 || !dist || (dist[12] == 0.0 && dist[13] == 0.0)) return;
    agt_side::tilt_matrices(dist[12], dist[13], t->m);
    t->on = 1;
}

}  // namespace

int hip_fail(agt_ctx* c, hipError_t e)
{
    if (c) c->last_hip = (int)e;
    g_last_hip = (int)e;
    (void)hipGetLastError();   // clear the sticky error so later launches are not blamed
    return AGT_ERR_HIP;
}

// camera of a call: intrinsics + the 12 polynomial coefficients by value; `tilt` (optional) receives the tilted-sensor matrices, the
// struct's device pointer stays null (camera_on: the form with the matrices in the context's device table)
int fill_camera(const double* K, const double* dist, int ndist, AgtCameraHost* cam, AgtTiltHost* tilt)
{
    if (!K) return AGT_ERR_ARG;
    if (!(ndist == 0 || ndist == 4 || ndist == 5 || ndist == 8 || ndist == 12 || ndist == 14)) return AGT_ERR_DIST;
    if (ndist > 0 && !dist) return AGT_ERR_ARG;
    cam->fx = K[0]; cam->fy = K[4]; cam->cx = K[2]; cam->cy = K[5];
    for (int i = 0; i < 12; i++) cam->k[i] = i < ndist ? dist[i] : 0.0;
    cam->tilt = nullptr;
    if (tilt) tilt_matrices(dist, ndist, tilt);
    return AGT_OK;
}

// ... for a launch of context c.  A tilted camera's matrices go to a slot of the context's device table (AGT_TILT_SLOTS x 18 doubles):
// slot 0 belongs to the tracker (written at agt_tracker_init, behind a stream synchronisation: the tracker's internal streams read
// it), slots 1.. serve the stateless calls round-robin -- a slot that already holds the same matrices is re-used without a copy, a new
// camera's copy is ordered on the context's stream behind every launch that read the slot's previous content.
int camera_on(agt_ctx* c, const double* K, const double* dist, int ndist, AgtCameraHost* cam, bool tracker)
{
    AgtTiltHost t;
    int rc = fill_camera(K, dist, ndist, cam, &t);
    if (rc || !t.on) return rc;
    if (!c->d_tilt) {
        if (hipMalloc((void**)&c->d_tilt, sizeof(double) * 18 * AGT_TILT_SLOTS) != hipSuccess) { (void)hipGetLastError(); return AGT_ERR_ALLOC; }
        memset(c->tilt_valid, 0, sizeof(c->tilt_valid));
    }
    int slot = 0;
    if (!tracker) {
        slot = -1;
        for (int i = 1; i < AGT_TILT_SLOTS; i++) if (c->tilt_valid[i] && !memcmp(c->tilt_host[i], t.m, sizeof(t.m))) { slot = i; break; }
        if (slot < 0) {
            c->tilt_next = c->tilt_next % (AGT_TILT_SLOTS - 1) + 1; slot = c->tilt_next;
            // an eighth distinct tilted camera recycles a slot: launches that read its old content may sit on ANY stream the context was
            // bound to (agt_set_stream) -- wait for the device once (a camera change of this kind is not a per-frame event)
            if (c->tilt_valid[slot] && hipDeviceSynchronize() != hipSuccess) return hip_fail(c, hipGetLastError());
            c->tilt_valid[slot] = 0;
        }
    }
    if (!c->tilt_valid[slot] || memcmp(c->tilt_host[slot], t.m, sizeof(t.m))) {
        memcpy(c->tilt_host[slot], t.m, sizeof(t.m));
        // (the copy is waited for, tracker slot or not: the slot may be re-used WITHOUT a copy by a later call on another stream -- agt_set_stream --
        // and by the tracker's internal streams, none of which is ordered behind this stream.  A new tilted camera is not a per-frame event.  ADVICE r5)
        hipError_t e = hipMemcpyAsync(c->d_tilt + 18 * slot, c->tilt_host[slot], sizeof(t.m), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return hip_fail(c, e);
        c->tilt_valid[slot] = 1;
    }
    cam->tilt = c->d_tilt + 18 * slot;
    return AGT_OK;
}

// grow the rings to `want` entries (pyramid levels >= 1, corners, status)
int ensure_ring(agt_ctx* c, int want)
{
    if (want > AGT_RING_MAX) return AGT_ERR_UNSUPPORTED;
    const size_t B = (size_t)c->cfg.max_streams, N = (size_t)c->cfg.max_points;
    for (int s = c->ring; s < want; s++) {
        bool ok = true;
        for (int l = 1; l <= c->eff_max_level && ok; l++)
            ok = hipMalloc((void**)&c->lmem[s][l], B * (size_t)level_bstride(c, l)) == hipSuccess;
        ok = ok && hipMalloc((void**)&c->corners[s], B * N * 2 * sizeof(float)) == hipSuccess;
        ok = ok && hipMalloc((void**)&c->status[s], B * N) == hipSuccess;
        ok = ok && hipMemsetAsync(c->status[s], 1, B * N, c->stream) == hipSuccess;
        if (!ok) { hip_fail(c, hipGetLastError()); return AGT_ERR_ALLOC; }      // partial entry is freed by agt_destroy
        c->ring = s + 1;
    }
    return AGT_OK;
}

// ---- the device's geometry (agt_kernels.h AgtChip), queried once per device.  Contexts may be created from several threads (one context per
// thread is the library's threading model): the table is filled under a mutex and read through an acquire load of the entry's state.  It has
// a fixed CHIP_MAX entries, far above any device count a node has (16 entries turned a valid device 16+ into hipErrorInvalidDevice);
// agt_create refuses a device index beyond it.
namespace {
constexpr int CHIP_MAX = 256;
AgtChip g_chip[CHIP_MAX];
std::atomic<int> g_chip_state[CHIP_MAX];       // 0 = not queried, 1 = valid, -1 = query failed
std::mutex g_chip_mutex;
}
static const AgtChip g_chip_default = { 256, 8, 3, "gfx950" };       // a whole MI355X

void agt_chip_from_props(int cus, const char* gcn_arch, AgtChip* out)
{
    memset(out, 0, sizeof(*out));
    out->cus = cus;
    size_t i = 0;
    for (; gcn_arch && gcn_arch[i] && gcn_arch[i] != ':' && i + 1 < sizeof(out->arch); i++) out->arch[i] = gcn_arch[i];
    out->arch[i] = 0;
    // gfx950: 32 CUs per XCD; workgroups are dealt round-robin to the XCDs of the partition.  A CU count that is not 32 x a power of
    // two (a CU mask, an unknown part) gets the plain block order: still correct, just not L2-aware.
    int x = cus / 32;
    out->xcds = (cus % 32 == 0 && (x == 1 || x == 2 || x == 4 || x == 8)) ? x : 1;
    out->xshift = out->xcds == 8 ? 3 : out->xcds == 4 ? 2 : out->xcds == 2 ? 1 : 0;
}

const AgtChip* agt_chip_of(int device)
{
    if (device < 0 || device >= CHIP_MAX) return nullptr;
    int st = g_chip_state[device].load(std::memory_order_acquire);
    if (st == 0) {
        std::lock_guard<std::mutex> lock(g_chip_mutex);
        st = g_chip_state[device].load(std::memory_order_relaxed);
        if (st == 0) {
            int ndev = 0;
            hipDeviceProp_t p;
            if (hipGetDeviceCount(&ndev) == hipSuccess && device < ndev && hipGetDeviceProperties(&p, device) == hipSuccess) {
                agt_chip_from_props(p.multiProcessorCount, p.gcnArchName, &g_chip[device]); st = 1;
            } else { (void)hipGetLastError(); st = -1; }
            g_chip_state[device].store(st, std::memory_order_release);
        }
    }
    return st == 1 ? &g_chip[device] : nullptr;
}

// (every launcher asks this once or twice per launch: while the process has only ever created contexts on ONE device -- the usual
// case -- the answer is that device's entry, without a runtime call.  g_chip_only: null = no context yet, a table entry = the one device so
// far, &g_chip_default used as the "several devices" mark; set with a compare-exchange in agt_create, read with one acquire load)
static std::atomic<const AgtChip*> g_chip_only{nullptr};

const AgtChip& agt_chip_current(void)
{
    const AgtChip* only = g_chip_only.load(std::memory_order_acquire);
    if (only && only != &g_chip_default) return *only;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return g_chip_default; }
    const AgtChip* c = agt_chip_of(dev);
    return c ? *c : g_chip_default;
}

// The library's streams are a PROCESS resource (round 6).  A process has four hardware queues and the runtime deals
// every new stream onto them round-robin; it does not hand a destroyed stream's place to the next one.  Contexts that each created and
// destroyed their own three streams therefore left the next context's streams wherever the deal happened to stand -- two of them on
// one queue sooner or later, and the split pipeline, which needs its pyramid / LK / LK / pose launches on four different queues, ran
// 1.5-1.8 x slower from then on.  Now a set of three highest-priority streams per device is created once, lent
// to the context that runs a split pipeline and taken back at agt_destroy; a second live context on the device gets a second set.
namespace {
struct MsPoolEntry { int device; hipStream_t s[3]; bool busy; };
std::vector<MsPoolEntry> g_ms_pool;
std::mutex g_ms_pool_mutex;
}
int ms_pool_acquire(int device, hipStream_t out[3])
{
    std::lock_guard<std::mutex> lock(g_ms_pool_mutex);
    for (size_t i = 0; i < g_ms_pool.size(); i++)
        if (!g_ms_pool[i].busy && g_ms_pool[i].device == device) {
            g_ms_pool[i].busy = true;
            for (int k = 0; k < 3; k++) out[k] = g_ms_pool[i].s[k];
            return (int)i;
        }
    // the LK launches are the long pole of a split-mode step and share the chip with the pyramid launches of the caller's stream, whose
    // short workgroups otherwise take every wave slot first: the library's streams get the highest priority
    MsPoolEntry e; e.device = device; e.busy = true;
    // (a stream belongs to the device that is current when it is created: the context's, whatever the calling thread has selected)
    int cur = device;
    if (hipGetDevice(&cur) != hipSuccess) return -1;
    if (cur != device && hipSetDevice(device) != hipSuccess) return -1;
    int pr_lo = 0, pr_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&pr_lo, &pr_hi);      // (the default or the lowest priority measured the same: profiles/r06_experiments.md)
    bool ok = true;
    for (int k = 0; k < 3 && ok; k++) {
        if (hipStreamCreateWithPriority(&e.s[k], hipStreamNonBlocking, pr_hi) != hipSuccess) {
            for (int q = 0; q < k; q++) (void)hipStreamDestroy(e.s[q]);
            ok = false;
        } else out[k] = e.s[k];
    }
    if (cur != device) (void)hipSetDevice(cur);
    if (!ok) return -1;
    g_ms_pool.push_back(e);
    return (int)g_ms_pool.size() - 1;
}
static void ms_pool_release(int slot)
{
    std::lock_guard<std::mutex> lock(g_ms_pool_mutex);
    if (slot >= 0 && slot < (int)g_ms_pool.size()) g_ms_pool[slot].busy = false;
}

int agt_version(void) { return AGT_VERSION; }

const char* agt_error_string(int code)
{
    switch (code) {
    case AGT_OK: return "ok";
    case AGT_ERR_ARG: return "invalid argument";
    case AGT_ERR_ALLOC: return "allocation failed";
    case AGT_ERR_DIST: return "unsupported distortion coefficient count (0, 4, 5, 8, 12 or 14)";
    case AGT_ERR_NPOINTS: return "bad point count";
    case AGT_ERR_HIP: return "HIP runtime error";
    case AGT_ERR_UNSUPPORTED: return "unsupported configuration";
    case AGT_ERR_STATE: return "bad context state";
    case AGT_ERR_CHAIN: return "a chained launch gave up waiting for corners (stream state frozen until agt_tracker_reset)";
    default: return "unknown error";
    }
}

int agt_device_info(const agt_ctx* c, int* cus, int* xcds, char* arch, size_t arch_cap)
{
    if (!c) return AGT_ERR_ARG;
    if (cus) *cus = c->chip.cus;
    if (xcds) *xcds = c->chip.xcds;
    if (arch && arch_cap) { strncpy(arch, c->chip.arch, arch_cap - 1); arch[arch_cap - 1] = 0; }
    return AGT_OK;
}

int agt_create(const agt_config* cfg, void* hip_stream, agt_ctx** out)
{
    if (!cfg || !out) return AGT_ERR_ARG;
    *out = nullptr;
    if (cfg->width <= 0 || cfg->height <= 0 || cfg->max_level < 0 || cfg->max_level >= AGT_MAX_LEVELS) return AGT_ERR_ARG;
    if (cfg->max_points <= 0 || cfg->max_points > 256) return AGT_ERR_NPOINTS;
    if (cfg->max_streams <= 0) return AGT_ERR_ARG;
    if (!agt_lk_window_supported(cfg->win)) return AGT_ERR_UNSUPPORTED;
    for (int i = 0; i < 8; i++) if (cfg->reserved[i] != 0) return AGT_ERR_ARG;
    hipError_t e = hipSetDevice(cfg->device);
    if (e != hipSuccess) return hip_fail(nullptr, e);
    // the library holds gfx950 code objects only: refuse any other device here, with a code, instead of failing at the first launch
    const AgtChip* chip = agt_chip_of(cfg->device);
    if (!chip) return hip_fail(nullptr, hipErrorInvalidDevice);
    if (strcmp(chip->arch, "gfx950") != 0) return AGT_ERR_UNSUPPORTED;
    agt_ctx* c = new (std::nothrow) agt_ctx;
    if (!c) return AGT_ERR_ALLOC;
    memset(c, 0, sizeof(*c));
    c->ms_pool_slot = -1;
    c->cfg = *cfg;
    c->chip = *chip;
    {   // first device of the process: remember it; a second one: from now on the launchers ask the runtime which device is current
        const AgtChip* seen = nullptr;
        if (!g_chip_only.compare_exchange_strong(seen, chip, std::memory_order_acq_rel) && seen != chip) g_chip_only.store(&g_chip_default, std::memory_order_release);
    }
    c->stream = (hipStream_t)hip_stream;
    // buildOpticalFlowPyramid level geometry + early stop
    int w = cfg->width, h = cfg->height;
    int win_w, win_h;
    agt_lk_window_size(cfg->win, &win_w, &win_h);
    for (int l = 0; l <= cfg->max_level; l++) {
        c->lw[l] = w; c->lh[l] = h;
        c->lpitch[l] = ((long)w + 63) & ~63L;
        c->eff_max_level = l;
        w = (w + 1) / 2; h = (h + 1) / 2;
        if (w <= win_w || h <= win_h) break;
    }
    const size_t B = (size_t)cfg->max_streams, N = (size_t)cfg->max_points;
    c->group = 1;
    const int ring0 = c->eff_max_level + 2 > AGT_SLOTS ? c->eff_max_level + 2 : AGT_SLOTS;
    bool ok = ensure_ring(c, ring0) == AGT_OK;
    c->live_ring = ring0;
    ok = ok && hipMalloc((void**)&c->lkerr, B * N * sizeof(float)) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->obj, N * 3 * sizeof(float)) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->pose, B * 6 * sizeof(double)) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->tstate, B * sizeof(AgtTrackState)) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->lk_done, (size_t)AGT_RING_MAX * B * sizeof(unsigned)) == hipSuccess;
    ok = ok && hipMemset(c->lk_done, 0, (size_t)AGT_RING_MAX * B * sizeof(unsigned)) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&c->fault_host, 256, hipHostMallocMapped) == hipSuccess;
    if (ok) { memset(c->fault_host, 0, 256); ok = hipHostGetDevicePointer((void**)&c->fault_dev, c->fault_host, 0) == hipSuccess; }
    if (ok) {
        c->hrec_host = (double*)((char*)c->fault_host + 64); c->hrec_dev = (double*)((char*)c->fault_dev + 64);
        c->hseq_host = (unsigned long long*)((char*)c->fault_host + 192); c->hseq_dev = (unsigned long long*)((char*)c->fault_dev + 192);
    }
    if (!ok) { hip_fail(nullptr, hipGetLastError()); agt_destroy(c); return AGT_ERR_ALLOC; }
    c->split.reset_history();
    c->pipeline = agt_step_supported(cfg->win) ? 1 : 0;
    c->opt.reproject = 0; c->opt.min_points = 8; c->opt.gate_px = 2.0;
    // knobs: fixed iteration counts (AGT_LK_MAX_COUNT=n AGT_LK_EPS=0) separate the per-iteration cost of the LK role from its per-frame cost
    c->lk_max_count = AGT_KNOB("AGT_LK_MAX_COUNT", 30); c->lk_eps = AGT_KNOB_F("AGT_LK_EPS", 0.01); c->lk_min_eig = 1e-4;
    c->lk_cap_cu = -1;                               // (the library's choice: agt_lk_occupancy_cu)
    *out = c;
    return AGT_OK;
}

int agt_destroy(agt_ctx* c)
{
    if (!c) return AGT_OK;
    (void)hipStreamSynchronize(c->stream);
    for (int s = 0; s < AGT_RING_MAX; s++) {
        for (int l = 1; l < AGT_MAX_LEVELS; l++) if (c->lmem[s][l]) (void)hipFree(c->lmem[s][l]);
        if (c->corners[s]) (void)hipFree(c->corners[s]);
        if (c->status[s]) (void)hipFree(c->status[s]);
    }
    if (c->ms_pool_slot >= 0) {                      // (also after an ms_init that stopped half-way: the slot and the events it did create)
        for (int i = 0; i < 3; i++) (void)hipStreamSynchronize(c->ms_stream[i]);
        for (int k = 0; k < SplitEvents::ROWS; k++) for (int i = 0; i < AGT_EV_SLOTS; i++) if (c->split.ev[k][i]) (void)hipEventDestroy(c->split.ev[k][i]);
        ms_pool_release(c->ms_pool_slot);            // (the streams go back to the process's pool: see ms_pool_acquire)
    }
    if (c->lkerr) (void)hipFree(c->lkerr);
    if (c->obj) (void)hipFree(c->obj);
    if (c->pose) (void)hipFree(c->pose);
    if (c->tstate) (void)hipFree(c->tstate);
    if (c->lk_done) (void)hipFree(c->lk_done);
    if (c->fault_host) (void)hipHostFree(c->fault_host);
    if (c->dense_partials) (void)hipFree(c->dense_partials);
    if (c->cons_buf) (void)hipFree(c->cons_buf);
    if (c->pred_hist) (void)hipFree(c->pred_hist);
    if (c->dense_done) (void)hipFree(c->dense_done);
    if (c->d_tilt) (void)hipFree(c->d_tilt);
    if (c->hcall_host) (void)hipHostFree(c->hcall_host);
    if (c->map1) (void)hipFree(c->map1);
    if (c->map2) (void)hipFree(c->map2);
    if (c->prof_ev) {
        for (size_t i = 0; i < (size_t)c->prof_cap * AGT_PROF_EVENTS; i++) (void)hipEventDestroy(c->prof_ev[i]);
        delete[] c->prof_ev;
        delete[] c->prof_dense;
    }
    delete c;
    return AGT_OK;
}

int agt_set_stream(agt_ctx* c, void* hip_stream)
{
    if (!c) return AGT_ERR_ARG;
    c->stream = (hipStream_t)hip_stream;
    return AGT_OK;
}

int agt_last_hip_error(const agt_ctx* c) { return c ? c->last_hip : g_last_hip; }

int agt_synchronize(agt_ctx* c)
{
    if (!c) return AGT_ERR_ARG;
    int rc = join_pipeline(c);            // flush frames still inside the software pipeline
    if (rc) return rc;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e);
    return *(volatile int*)c->fault_host ? AGT_ERR_CHAIN : AGT_OK;
}

int agt_upload(agt_ctx* c, void* d_dst, const void* h_src, size_t bytes)
{
    if (!c || !d_dst || !h_src) return AGT_ERR_ARG;
    hipError_t e = hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c->stream);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

int agt_download(agt_ctx* c, void* h_dst, const void* d_src, size_t bytes)
{
    if (!c || !h_dst || !d_src) return AGT_ERR_ARG;
    hipError_t e = hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}
