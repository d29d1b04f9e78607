// What the api*.cpp translation units share: the per-thread context with its workspaces, the handle types, and the helpers
// more than one entry-point family calls.  All state is defined once, in api_ctx.cpp; nothing here is part of the C ABI.
#pragma once
#include <sched.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "kernels.h"

namespace tdtk {

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                          \
      return TDTK_EDEVICE;                                                                   \
    }                                                                                        \
  } while (0)

// ------------------------------------------------------------------------------------------
// per-thread, per-device context: stream, events, growable workspaces
// ------------------------------------------------------------------------------------------
// the arrays of trees and resident scans and the per-context workspaces below come from the pool (pool.cpp)
hipError_t handle_malloc(void** p, size_t bytes);

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) pool_free(p); }     // (pooled like the handles' arrays: the contexts of a prefetch pool's threads come and go)
  int ensure(size_t bytes)
  {
    if (bytes <= cap) return TDTK_OK;
    if (p) pool_free(p);
    p = nullptr; cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = (hipError_t)pool_malloc_raw(&p, want);
    if (e != hipSuccess) { set_error(std::string("hipMalloc: ") + hipGetErrorString(e)); return TDTK_ENOMEM; }
    cap = want;
    return TDTK_OK;
  }
  template <class T> T* as() { return static_cast<T*>(p); }
};

enum { WS_KPOS, WS_D2, WS_PART, WS_OUT, WS_OVF_M2, WS_OVF_REF, WS_IDX, WS_QX, WS_QY, WS_QZ, WS_DX,
       WS_DY, WS_DZ, WS_ORDER, WS_CELL, WS_HIST, WS_TMPA, WS_TMPB, WS_CNT, WS_BOX, WS_ARENA, WS_COST, WS_MOVES, WS_BOUNDS, WS_CERT, WS_COUNT };

// an auxiliary stream with the buffers one whole-scan pass needs: batches of links over small scans run several
// passes side by side (one pass of an 80K-point scan occupies a fraction of the machine and is latency-bound)
// draw counters of the work-queue search kernel: two sets of 8 that alternate from launch to launch on one stream
// (each launch zeroes the set of the next one, kernels.hip)
struct QueueCtr {
  DevBuf buf;
  int parity = 0;
  int attach(SearchArgs& a)
  {
    if (!buf.p) {
      int rc = buf.ensure(64 * sizeof(uint32_t));
      if (rc) return rc;
      if (hipMemset(buf.p, 0, 64 * sizeof(uint32_t)) != hipSuccess) { set_error("hipMemset failed"); return TDTK_EDEVICE; }
    }
    a.q_ctr = buf.as<uint32_t>() + 32 * parity;
    a.q_ctr_next = buf.as<uint32_t>() + 32 * (parity ^ 1);
    parity ^= 1;
    return TDTK_OK;
  }
};

struct Lane {
  hipStream_t s = nullptr;
  bool owns = true;     // lane 0 runs on the context's own stream
  QueueCtr qc;
  DevBuf kpos, part, ovf_m2, ovf_ref;
  DevBuf moved;      // batched link passes: this link's own copy of a scan another link of the launch is moving (lazy moves)
  // batched link passes: whose hits kpos holds (handle numbers of the tree and the scan, queries) -- the next pass of the SAME
  // link at this position starts every search from its previous hit (SearchArgs::warm)
  uint64_t k_tree = 0, k_scan = 0; size_t k_n = 0;
  ~Lane() { if (s && owns) (void)hipStreamDestroy(s); }
};

// batched link passes: what each query of the link at this position of the launch order cost in the previous pass (one
// byte per query: the next pass's hand-out order), and which link that was
struct LinkCost {
  DevBuf cost;
  const void* tree = nullptr; const void* scan = nullptr; size_t n = 0;
};

struct Ctx {
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;   // around the search kernel of the last pass
  hipEvent_t e2 = nullptr, e3 = nullptr;   // around the pair-sum kernels behind it (k_accum + k_final, or k_final alone)
  hipEvent_t e4 = nullptr, e5 = nullptr;   // around k_ann_normals of the last calcNormals
  hipEvent_t e_user = nullptr;             // fence between a caller's stream and this context's stream
  hipEvent_t e_defer = nullptr;            // behind the last batch of scan moves that was left running (defer_fence)
  hipStream_t stream_b = nullptr, stream_c = nullptr, stream_d = nullptr;   // the tree build's background chains (exact centroid sums beside the levels below)
  hipEvent_t e_b1 = nullptr, e_b2 = nullptr, e_b3 = nullptr, e_b4 = nullptr;
  DevBuf ws[WS_COUNT];
  double* h_pin = nullptr;  // pinned staging for the per-iteration sums: words [0, ACC_TOTAL); behind them two slots of the tree build
  // (both are filled by copies enqueued on `stream` and read only behind a synchronisation of that stream that was made after
  //  the copy was enqueued: one of the build's looks at the device for the box, tree_finish's own hipStreamSynchronize for the
  //  groups -- device_build_tree may return with its last kernels still running, see build.hip "no_last_look")
  static constexpr int PIN_BOX = 128;      // 7 doubles: the root bounding box and the non-finite flag (tree_from_device_points)
  static constexpr int PIN_GROUPS = 140;   // 1 uint32: groups of the padded layout (tree_pad_buckets -> tree_finish)
  static constexpr int PIN_OCT_RANGE = 144;   // 1 uint32: the range word of an octree ICP iteration, copied ahead of its sums
  void* h_build = nullptr;  // 64 KB, pinned: the tree build's looks at the device (BuildSide::h_pin)
  void* h_stage = nullptr;  // pinned staging for descriptor tables of batched launches (grows on demand)
  size_t h_stage_cap = 0;
  DevBuf d_mask, d_skip;                // -R passes: the keep-mask (bits, caller order) and what the search reads (bytes, sorted order)
  std::vector<unsigned char> h_mask;
  DevBuf d_loop;                        // lab, the host-free ICP loop: its IcpLoopDev block (kernels.h)
  double* h_loop = nullptr;             // ... and its record, pinned: ICP_LOOP_RING rows of ICP_ROW doubles
  DevBuf d_hash;                        // tdtk_icp_index_hashes: one 64-bit word per iteration of the last tdtk_icp_match
  std::vector<uint64_t> last_hashes;
  void* h_moves = nullptr;  // pinned staging of scans_settle's table (its own: a settle may precede a batched launch in one call)
  size_t h_moves_cap = 0;
  hipEvent_t e_moves = nullptr;   // behind the last copy out of h_moves
  bool moves_inflight = false;
  double last_nn_ms = 0.0, last_sums_ms = 0.0, last_normals_ms = 0.0, last_build_ms = 0.0;
  bool ev_pending = false, ev2_pending = false, ev4_pending = false;
  uint64_t counted_ann_queries = 0;
  // tdtk_visit_counting: every search of this thread runs its instrumented instantiation and adds to d_counters
  bool counting = false;
  // tdtk_visit_counting(device, 2): count the REFERENCE's walk -- every search while counting starts cold (no warm start, no
  // deferred quick check), i.e. kdTreeImpl.h:345-383 with radius maxdist2; results are the same, so a loop stays on its path
  bool count_cold = false;
  DevBuf d_counters;
  uint64_t counted_queries = 0;
  std::vector<std::unique_ptr<Lane>> lanes;
  std::vector<std::unique_ptr<Lane>> slots;   // per-link buffers of a several-links-in-one-launch batch (no streams)
  std::vector<std::unique_ptr<LinkCost>> link_costs;
  DevBuf multi_args;                          // its argument tables on the device
  std::vector<void*> free_later;              // see pool_free_later
  QueueCtr qc;       // for launches on `stream` (a caller's stream gets its launches ordered behind it, see run_search)
  // slabs of equal cost for the next pass of an ICP loop (launch_slab_bounds): valid for the loop's next scan_pass only
  const uint32_t* next_bounds = nullptr;
  size_t next_bounds_n = 0;
  // WS_CERT holds the certificates (SearchArgs::cert) the last scan_pass of the running tdtk_icp_match loop wrote for exactly
  // the queries and the tree of its next pass: set by a pass that wrote them, cleared by every other pass and where a loop starts
  bool cert_live = false;
  // the Hough transform's own buffers (api_hough.cpp): the cloud of the last call that uploaded one, the last vote's table and
  // counts -- kept from call to call, so a Hough object's steps upload the cloud once and peaks read the vote's counts in place
  DevBuf hough_xyz, hough_normals, hough_counts, hough_rho;
  size_t hough_n = 0, hough_cells = 0;
  uint32_t hough_rho_num = 0;
  bool hough_have_xyz = false, hough_have_counts = false;
  // a context dies with its host thread (worker threads of a prefetch pool come and go): give everything back
  ~Ctx();
};

// Batched scan moves (the pose update of a graph-SLAM round: every resident scan of the rank, ~0.6 ms for 63 x 1M
// points) are left running when the call returns; whatever the host does next -- Python marshalling, building the
// next round's graph -- overlaps with them.  The fence is process-wide: the next library call of ANY host thread on
// that device waits for it in get_ctx before it touches a scan, so "the scans have moved when the call has returned"
// still holds for everything that can observe them.
struct Deferred { int device; hipEvent_t ev; Ctx* owner; };

// ---- state (api_ctx.cpp) --------------------------------------------------------------------
extern std::atomic<int> g_ctx_live;             // host threads that hold a context right now (all devices)
extern std::atomic<uint64_t> g_respeculated;   // tree builds whose speculative cuts failed the final check
extern std::atomic<uint64_t> g_handle_uid;     // the next tree / scan handle's number
extern std::recursive_mutex g_moves_mu;        // guards every scan's pending / npend / ax..az and the x <-> ax swap
extern std::atomic<int> g_kernel_timing;       // api_search.cpp: kernel_timing
extern std::atomic<int> g_icp_hashes;          // api_icp.cpp: tdtk_icp_index_hashes
extern thread_local std::vector<uint64_t> t_last_hashes;
// longest chain a scan may carry: a rank that never reads a scan (seven of eight ranks, for most scans) carries it out
// once per this many queued transforms -- one trip of the points through HBM per 16 rounds instead of one per round
constexpr size_t LAZY_CHAIN_MAX = 32;

// ---- helpers of more than one family, by the file that defines them -------------------------
// api_ctx.cpp
double now_ms();
void wait_deferred(int device, const Ctx* only_owner = nullptr);
int get_ctx(int device, Ctx** out, bool touches_scans = true);
int defer_fence(Ctx* c);
int stage_reserve(Ctx* c, size_t bytes);
int stage_pinned(Ctx* c, const void* src, size_t bytes, void** out);
int scan_keep_original(Ctx* c, tdtk_scan* s);
bool lazy_moves();
int scans_settle(Ctx* c, const tdtk_scan* const* scans, int count);
int scan_settle(Ctx* c, const tdtk_scan* s);
int scan_ensure_spare(const tdtk_scan* sc);
void scan_queue_move(tdtk_scan* s, const double* A16);
// api_tree.cpp
int tree_from_device_points(Ctx* c, tdtk_tree* t, size_t M, int bucket_size, double t0);
int tree_finish(Ctx* c, tdtk_tree* t, size_t M);
int tree_check_args(size_t M, int bucket_size);
// api_query.cpp
int adaptive_check_args(const double* xyz, size_t n, int kmin, int kmax, const double* rPos, const double* normals_out);
struct QueryArgs;
int query_prepare(Ctx* c, const tdtk_tree* t, const double* d_q, size_t K, QueryArgs& a, const double* d_v = nullptr,
                  const double* box = nullptr, size_t n_walks = 0);   // (also the forest's queries, api_forest.cpp: t a stand-in that carries max_depth)
int knn_check_k(int k);
// count walk, scan, offsets to the host, capacity check, fill walk, downloads: every list query, a tree's or the forest's
int list_walks(Ctx* c, const char* name, const char* noun, QueryArgs& a, bool timed, const std::function<int()>& count,
               const std::function<int()>& fill, uint64_t* offsets, int32_t* idx, double* d2, size_t cap, uint64_t* total);
// api_search.cpp
constexpr uint64_t SUMS_ARMED = 0x7FF8DEADBEEF0001ull;   // a NaN no sum can produce: the word a host arms before it watches for a result
int prepare_overflow_in(DevBuf& bm2, DevBuf& bref, const tdtk_tree* t, size_t nq, SearchArgs& a);
bool kernel_timing();
int run_search(Ctx* c, const tdtk_tree* t, SearchArgs& a, int dirmode, bool count, hipStream_t s, bool timed);
int collect_ms(Ctx* c, double* ms, double* sums_ms = nullptr);
int fuse_mode(size_t N);
void finish_sums(const double* acc, const double shift[3], size_t nq, unsigned want, tdtk_pair_sums* o);
double search_margin(const tdtk_tree* t, double maxd2);
void pass_shift(const tdtk_tree* t, const double* A16, double out[3]);
int scan_pass(Ctx* c, const tdtk_tree* model, const double* A16, tdtk_scan* data, int pmode, double maxd2,
              unsigned want, const double* lum_D, const double* pending, bool do_search, double* acc_out,
              double shift_out[3], bool warm = false, const unsigned char* skip = nullptr, bool cert_ok = false);
int scan_idx_to_host(Ctx* c, const tdtk_tree* model, tdtk_scan* data, int32_t* idx_out);
// api_icp.cpp
// icp6D::match's loop (tdtk_icp_match) over a search tree that is not the k-d tree: `model` stands in for it where the loop
// needs a tdtk_tree (the device, the point array the index hashes read), and one iteration's search and sums are the pass's:
// it applies `pending` (the previous iteration's alignxf, nullable) to the scan, searches -- `skip`: the -R keep bytes,
// nullable -- and leaves the raw sums in acc [ACC_TOTAL] about shift, the hits in WS_KPOS.  `check` runs behind the argument
// checks and before anything moves.  A pass that fails ends the loop with res->iterations = its iteration.
struct IcpTreePass {
  std::function<int(int pmode, double maxd2)> check;
  std::function<int(const double* pending, const unsigned char* skip, unsigned want, double* acc, double shift[3])> pass;
};
int icp_match_loop(const tdtk_tree* model, const IcpTreePass* other, const double model_dalignxf[16], tdtk_scan* data,
                   double data_transMat[16], double data_dalignxf[16], const tdtk_icp_params* prm, int rnd,
                   tdtk_icp_result* res, double* trace, int trace_cap);
// api_scan.cpp
int queue_scan_moves(Ctx* c, const std::vector<tdtk_scan*>& moved);
using PairsPass = std::function<int(tdtk_scan*, int32_t*, tdtk_pair_sums*)>;
int get_pt_pairs_over(const tdtk_tree* t, const PairsPass& pairs, const double A[16], const double* xyz_r, const double* normal_r,
                      size_t start, size_t end, int rnd, int pmode, double maxd2, uint32_t want,
                      int32_t* idx_out, double* p1_out, double* p2_out, double* pn_out, tdtk_pair_sums* sums);

}  // namespace tdtk

// ------------------------------------------------------------------------------------------
// handles
// ------------------------------------------------------------------------------------------
struct tdtk_tree {
  const uint64_t uid = tdtk::g_handle_uid.fetch_add(1, std::memory_order_relaxed);
  int device = 0;
  size_t M = 0;
  int bucket = 0;
  tdtk::TreeDev dev{};
  void *d_nodes = nullptr, *d_pts = nullptr, *d_leaf = nullptr, *d_r = nullptr, *d_hot = nullptr, *d_grp = nullptr, *d_fat = nullptr;
  void* d_q16 = nullptr;     // 16-bit shadow of the padded buckets (TreeDev::q16), 6 bytes per slot + 128 of slack
  void* d_split = nullptr;   // { splitval, children } of every internal node, 16 bytes (TreeDev::split): inside d_hot's allocation
  double q_lo[3] = {0, 0, 0}, q_scale = 0.0;
  size_t Mp = 0;   // slots of d_pts: M, or 4 * groups once the buckets are padded to whole groups (tree_pad_buckets)
  double bbmin[3], bbmax[3], centre[3];
  tdtk_tree_info info{};
  uint32_t build_path[12] = {0xFFFFFFFFu};   // tdtk_tree_build_path: what the device build decided (BuildPath); as it stands: no device build
  tdtk_tree() = default;
  tdtk_tree(const tdtk_tree&) = delete;
  tdtk_tree& operator=(const tdtk_tree&) = delete;
  ~tdtk_tree()   // also the error paths of tdtk_tree_create: nothing stays allocated on the device
  {
    (void)hipSetDevice(device);
    void* p[] = {d_nodes, d_pts, d_leaf, d_r, d_hot, d_grp, d_fat, d_q16};
    for (void* q : p)
      if (q) tdtk::pool_free(q);
  }
};

struct tdtk_scan {
  const uint64_t uid = tdtk::g_handle_uid.fetch_add(1, std::memory_order_relaxed);
  int device = 0;
  size_t N = 0;
  double *x = nullptr, *y = nullptr, *z = nullptr, *nx = nullptr, *ny = nullptr, *nz = nullptr;
  int32_t* d_order = nullptr;    // sorted position -> caller index
  // "xyz reduced original" (basicScan.cc:739-757 copyReducedToOriginal): once tdtk_scan_mark_original has been
  // called, the first operation that moves the points first saves them here (a device-to-device copy), so the
  // scan's search tree can still be built later without the points ever visiting the host
  bool track_original = false;
  double *ox = nullptr, *oy = nullptr, *oz = nullptr;
  // Lazy moves.  The pose update of a graph-SLAM round does not touch the points: it queues its in-place transforms here
  // (oldest first), and whoever reads the scan next applies them -- the link passes of the next round in registers where a
  // lane takes a query (the link that owns the update stores the result into the spare arrays ax / ay / az, swapped in
  // behind the launch), every other entry point through scan_settle (one pass, all queued matrices in order).  A rank
  // never moves a scan none of its links reads.  The arithmetic is the one Scan::transform does point by point
  // (scan.cc:851-875), matrix after matrix: same bits as moving the scan every time.
  // Several host threads may hold the same scan (a prefetch pool, an OpenMP host): the queue, the spare arrays and the
  // swap are only touched under g_moves_mu; npend mirrors pending.size() so that the readers' fast path ("nothing
  // queued") takes no lock.  A settle issued while more than one context is live waits for its kernel before it
  // publishes npend == 0, so a reader on ANOTHER stream that finds nothing queued also finds the points moved.
  mutable std::vector<tdtk::Mat4> pending;
  mutable std::atomic<uint32_t> npend{0};
  mutable double *ax = nullptr, *ay = nullptr, *az = nullptr;
  tdtk_scan() = default;
  tdtk_scan(const tdtk_scan&) = delete;
  tdtk_scan& operator=(const tdtk_scan&) = delete;
  ~tdtk_scan()
  {
    (void)hipSetDevice(device);
    double* p[] = {x, y, z, nx, ny, nz, ox, oy, oz, ax, ay, az};
    for (double* q : p)
      if (q) tdtk::pool_free(q);
    if (d_order) tdtk::pool_free(d_order);
  }
};
