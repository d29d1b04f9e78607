// C ABI of lib3dtk_hip.so (include/tdtk_hip.h), host side: errors, the per-thread context, the deferred fence, pinned staging and
// lazy scan moves, with ALL state of the api*.cpp files -- defined here once and in this order (Ctx::~Ctx takes g_defer_mu and
// walks g_defer when a thread exits).  There is NO CPU fallback in this library: without a HIP device every compute entry point
// fails with TDTK_EDEVICE.
#include "api_internal.h"

using namespace tdtk;

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err;
void tdtk::set_error(const std::string& s) { g_err = s; }

namespace tdtk {

std::atomic<int> g_ctx_live{0};             // host threads that hold a context right now (all devices)
std::atomic<uint64_t> g_respeculated{0};   // tree builds whose speculative cuts failed the final check

double now_ms()
{
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

hipError_t handle_malloc(void** p, size_t bytes) { return (hipError_t)pool_malloc_raw(p, bytes); }

static std::mutex g_defer_mu;
static std::atomic<int> g_defer_n{0};
static std::vector<Deferred> g_defer;

void wait_deferred(int device, const Ctx* only_owner)
{
  if (g_defer_n.load(std::memory_order_acquire) == 0) return;
  std::lock_guard<std::mutex> lk(g_defer_mu);
  for (size_t i = 0; i < g_defer.size();) {
    if (g_defer[i].device == device && (!only_owner || g_defer[i].owner == only_owner)) {
      (void)hipEventSynchronize(g_defer[i].ev);
      g_defer.erase(g_defer.begin() + (long)i);
    } else {
      ++i;
    }
  }
  g_defer_n.store((int)g_defer.size(), std::memory_order_release);
}

Ctx::~Ctx()
  {
    g_ctx_live.fetch_sub(1);
    if (device >= 0) (void)hipSetDevice(device);
    wait_deferred(device, this);
    if (e_defer) (void)hipEventDestroy(e_defer);
    for (void* q : free_later) pool_free(q);
    free_later.clear();
    if (h_stage) (void)hipHostFree(h_stage);
    if (h_moves) (void)hipHostFree(h_moves);
    if (e_moves) (void)hipEventDestroy(e_moves);
    lanes.clear();
    slots.clear();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e2) (void)hipEventDestroy(e2);
    if (e3) (void)hipEventDestroy(e3);
    if (e4) (void)hipEventDestroy(e4);
    if (e5) (void)hipEventDestroy(e5);
    if (e_user) (void)hipEventDestroy(e_user);
    if (e_b1) (void)hipEventDestroy(e_b1);
    if (e_b2) (void)hipEventDestroy(e_b2);
    if (e_b3) (void)hipEventDestroy(e_b3);
    if (e_b4) (void)hipEventDestroy(e_b4);
    if (stream_b) (void)hipStreamDestroy(stream_b);
    if (stream_c) (void)hipStreamDestroy(stream_c);
    if (stream_d) (void)hipStreamDestroy(stream_d);
    if (h_pin) (void)hipHostFree(h_pin);
    if (h_loop) (void)hipHostFree(h_loop);     // (lab)
    if (h_build) (void)hipHostFree(h_build);
    if (stream) (void)hipStreamDestroy(stream);
  }

static thread_local std::map<int, std::unique_ptr<Ctx>> g_ctx;

int get_ctx(int device, Ctx** out, bool touches_scans)
{
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_error("no HIP device available (lib3dtk_hip has no CPU fallback)");
    return TDTK_EDEVICE;
  }
  if (device < 0 || device >= ndev) { set_error("bad device ordinal"); return TDTK_EINVAL; }
  HIPCHK(hipSetDevice(device));
  auto it = g_ctx.find(device);
  if (it == g_ctx.end()) {
    std::unique_ptr<Ctx> c(new Ctx);
    c->device = device;
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&c->e0));
    HIPCHK(hipEventCreate(&c->e1));
    HIPCHK(hipEventCreate(&c->e2));
    HIPCHK(hipEventCreate(&c->e3));
    HIPCHK(hipEventCreate(&c->e4));
    HIPCHK(hipEventCreate(&c->e5));
    HIPCHK(hipEventCreateWithFlags(&c->e_user, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->e_defer, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->e_moves, hipEventDisableTiming));
    // (coherent, said explicitly: the host reads these words while the kernel that writes them is still running -- await_sums)
    HIPCHK(hipHostMalloc((void**)&c->h_pin, sizeof(double) * 256, hipHostMallocCoherent));
    HIPCHK(hipHostMalloc(&c->h_build, 65536, hipHostMallocDefault));
    it = g_ctx.emplace(device, std::move(c)).first;
    g_ctx_live.fetch_add(1);
  }
  *out = it->second.get();
  if (touches_scans) wait_deferred(device);    // (the timing / counter read-outs do not: they must not end the overlap)
  return TDTK_OK;
}

int ctx_stream(int device, void** stream_out)
{
  Ctx* c;
  int rc = get_ctx(device, &c);
  if (rc) return rc;
  *stream_out = c->stream;
  return TDTK_OK;
}

// leave what has been enqueued on c->stream running (see Deferred); TDTK_SYNC_MOVES=1 waits as before
int defer_fence(Ctx* c)
{
  static const bool sync_moves = [] { const char* e = getenv("TDTK_SYNC_MOVES"); return e && e[0] == '1'; }();
  if (sync_moves) { HIPCHK(hipStreamSynchronize(c->stream)); return TDTK_OK; }
  // the event is re-recorded under the lock: another host thread may be inside hipEventSynchronize on this very event
  // (wait_deferred holds the lock while it waits), and re-recording an event somebody is waiting on is undefined
  std::lock_guard<std::mutex> lk(g_defer_mu);
  HIPCHK(hipEventRecord(c->e_defer, c->stream));
  bool have = false;
  for (const Deferred& d : g_defer) have = have || d.owner == c;
  if (!have) g_defer.push_back({c->device, c->e_defer, c});
  g_defer_n.store((int)g_defer.size(), std::memory_order_release);
  return TDTK_OK;
}

// pinned host staging that stays valid until the next library call on this thread (get_ctx has then waited for the
// copy that reads it)
int stage_reserve(Ctx* c, size_t bytes)
{
  if (c->h_stage_cap < bytes) {
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    c->h_stage = nullptr; c->h_stage_cap = 0;
    const size_t want = std::max<size_t>(bytes, 64 * 1024);
    if (hipHostMalloc(&c->h_stage, want, hipHostMallocDefault) != hipSuccess) { set_error("hipHostMalloc failed"); return TDTK_ENOMEM; }
    c->h_stage_cap = want;
  }
  return TDTK_OK;
}
int stage_pinned(Ctx* c, const void* src, size_t bytes, void** out)
{
  int rc = stage_reserve(c, bytes);
  if (rc) return rc;
  std::memcpy(c->h_stage, src, bytes);
  *out = c->h_stage;
  return TDTK_OK;
}

// every tree / scan handle of the process has a number of its own: what "the same tree, the same scan as last time" is tested
// with where a stale answer would be an out-of-range read (a freed handle's address can come back)
std::atomic<uint64_t> g_handle_uid{1};

// copy-on-first-write of a tracked scan's original points; called by everything that moves a resident scan
int scan_keep_original(Ctx* c, tdtk_scan* s)
{
  if (!s || !s->track_original || s->ox || s->N == 0) return TDTK_OK;
  const size_t b = s->N * sizeof(double);
  {   // all three or none (a partial set would pass the `s->ox` test above next time)
    void* p[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; k++)
      if (handle_malloc(&p[k], b) != hipSuccess) {
        for (int j = 0; j < k; j++) pool_free(p[j]);
        set_error("out of device memory (saved original of a scan)");
        return TDTK_ENOMEM;
      }
    s->ox = static_cast<double*>(p[0]); s->oy = static_cast<double*>(p[1]); s->oz = static_cast<double*>(p[2]);
  }
  HIPCHK(hipMemcpyAsync(s->ox, s->x, b, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(s->oy, s->y, b, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(s->oz, s->z, b, hipMemcpyDeviceToDevice, c->stream));
  return TDTK_OK;
}

// ---- lazy scan moves (see tdtk_scan::pending) ---------------------------------------------------
std::recursive_mutex g_moves_mu;      // guards every scan's pending / npend / ax..az and the x <-> ax swap
bool lazy_moves()
{
  const char* e = getenv("TDTK_LAZY_MOVES");     // 0: every queued move is carried out at once (the round-3 behaviour)
  return !(e && e[0] == '0');
}

// carry out what is queued on these scans: one launch, every scan's chain in order.  Enqueued on c->stream; the caller
// decides whether to wait (the entry points that go on to read the scan on the same stream need not).
int scans_settle(Ctx* c, const tdtk_scan* const* scans, int count)
{
  {   // fast path without the lock: nothing queued on any of them
    bool any = false;
    for (int i = 0; i < count && !any; i++) any = scans[i] && scans[i]->npend.load(std::memory_order_acquire) != 0;
    if (!any) return TDTK_OK;
  }
  std::lock_guard<std::recursive_mutex> lk(g_moves_mu);
  size_t nmat = 0, max_n = 0;
  int nd = 0;
  for (int i = 0; i < count; i++) {
    const tdtk_scan* sc = scans[i];
    if (!sc || sc->pending.empty()) continue;
    bool dup = false;
    for (int j = 0; j < i && !dup; j++) dup = scans[j] == sc;
    if (dup) continue;
    if (!sc->N) { sc->pending.clear(); sc->npend.store(0, std::memory_order_release); continue; }
    if (sc->device != c->device) { set_error("resident scans of one call must live on one device"); return TDTK_EINVAL; }
    nmat += sc->pending.size(); nd++;
    max_n = std::max(max_n, sc->N);
  }
  if (!nd) {
    for (int i = 0; i < count; i++)
      if (scans[i] && scans[i]->pending.empty()) scans[i]->npend.store(0, std::memory_order_release);
    return TDTK_OK;
  }
  const size_t o_mat = ((sizeof(XfChainDesc) * (size_t)nd + 127) / 128) * 128, bytes = o_mat + nmat * sizeof(Mat4);
  int rc = c->ws[WS_MOVES].ensure(bytes);
  if (rc) return rc;
  if (c->moves_inflight) { HIPCHK(hipEventSynchronize(c->e_moves)); c->moves_inflight = false; }
  if (c->h_moves_cap < bytes) {
    if (c->h_moves) (void)hipHostFree(c->h_moves);
    c->h_moves = nullptr; c->h_moves_cap = 0;
    const size_t want = std::max<size_t>(bytes + bytes / 2, 64 * 1024);
    if (hipHostMalloc(&c->h_moves, want, hipHostMallocDefault) != hipSuccess) { set_error("hipHostMalloc failed"); return TDTK_ENOMEM; }
    c->h_moves_cap = want;
  }
  char* tab = static_cast<char*>(c->h_moves);
  std::memset(tab, 0, o_mat);
  XfChainDesc* hd = reinterpret_cast<XfChainDesc*>(tab);
  Mat4* hm = reinterpret_cast<Mat4*>(tab + o_mat);
  const Mat4* dm = reinterpret_cast<const Mat4*>(static_cast<char*>(c->ws[WS_MOVES].p) + o_mat);
  size_t k = 0;
  std::vector<const tdtk_scan*> moved;      // (each scan once, however often the caller's list names it)
  for (int i = 0; i < count; i++) {
    const tdtk_scan* sc = scans[i];
    if (!sc || sc->pending.empty() || std::find(moved.begin(), moved.end(), sc) != moved.end()) continue;
    XfChainDesc& e = hd[moved.size()];
    e.x = sc->x; e.y = sc->y; e.z = sc->z; e.nx = sc->nx; e.ny = sc->ny; e.nz = sc->nz; e.n = sc->N;
    e.mats = dm + k; e.nm = (int)sc->pending.size();
    for (const Mat4& m : sc->pending) hm[k++] = m;
    moved.push_back(sc);
  }
  // The queues are emptied -- chain and count together -- only once the chain kernel is on the stream: a copy, an event or a
  // launch that fails on the way returns with every move still queued (round-5 advice: they used to be lost).
  HIPCHK(hipMemcpyAsync(c->ws[WS_MOVES].p, tab, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipEventRecord(c->e_moves, c->stream));
  c->moves_inflight = true;
  HIPCHK(launch_transform_chain_batch(reinterpret_cast<const XfChainDesc*>(c->ws[WS_MOVES].p), (int)moved.size(), max_n, c->stream));
  for (const tdtk_scan* sc : moved) sc->pending.clear();
  // other contexts (host threads with streams of their own) may read these scans next: they must not find "nothing
  // queued" before the chain kernel has run.  A lone context orders everything on its one stream and need not wait.
  if (g_ctx_live.load() > 1) HIPCHK(hipStreamSynchronize(c->stream));
  for (int i = 0; i < count; i++)
    if (scans[i] && scans[i]->pending.empty()) scans[i]->npend.store(0, std::memory_order_release);
  return TDTK_OK;
}
int scan_settle(Ctx* c, const tdtk_scan* s)
{
  if (!s || s->npend.load(std::memory_order_acquire) == 0) return TDTK_OK;
  return scans_settle(c, &s, 1);
}
// the spare coordinate arrays of a scan (tdtk_scan::ax / ay / az): all three or none -- a launch stores through all of
// them and swaps them in, so a partial set (one allocation of the three failed) must never be left on the handle
int scan_ensure_spare(const tdtk_scan* sc)
{
  if (sc->ax && sc->ay && sc->az) return TDTK_OK;
  const size_t b = sc->N * sizeof(double);
  void* p[3] = {nullptr, nullptr, nullptr};
  for (int k = 0; k < 3; k++) {
    if (handle_malloc(&p[k], b) != hipSuccess) {
      for (int j = 0; j < k; j++) pool_free(p[j]);
      set_error("out of device memory (spare arrays of a moving scan)");
      return TDTK_ENOMEM;
    }
  }
  double* old[3] = {sc->ax, sc->ay, sc->az};
  for (double* q : old)
    if (q) pool_free(q);
  sc->ax = static_cast<double*>(p[0]); sc->ay = static_cast<double*>(p[1]); sc->az = static_cast<double*>(p[2]);
  return TDTK_OK;
}
// queue one in-place transform on a resident scan (the caller has saved "xyz reduced original" if it is tracked)
void scan_queue_move(tdtk_scan* s, const double* A16)
{
  Mat4 m;
  std::memcpy(m.m, A16, sizeof m.m);
  std::lock_guard<std::recursive_mutex> lk(g_moves_mu);
  s->pending.push_back(m);
  s->npend.store((uint32_t)s->pending.size(), std::memory_order_release);
}

// switches of single families, kept with the rest of the state
std::atomic<int> g_kernel_timing{-1};     // api_search.cpp: kernel_timing
std::atomic<int> g_icp_hashes{0};         // api_icp.cpp: tdtk_icp_index_hashes
// the words of the calling thread's last tdtk_icp_match, whatever device it ran on (no context is looked up, none created)
thread_local std::vector<uint64_t> t_last_hashes;

}  // namespace tdtk

// ------------------------------------------------------------------------------------------
extern "C" {

const char* tdtk_last_error(void) { return g_err.c_str(); }
const char* tdtk_version(void) { return "3dtk_amd 0.1 (gfx950)"; }

size_t tdtk_pool_trim(void) { return pool_trim(); }
uint64_t tdtk_build_respeculated(void) { return g_respeculated.load(); }

int tdtk_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

}  // extern "C"
