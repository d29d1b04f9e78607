// The kd-tree handle: device construction, padding of the buckets, the search-side records; the tdtk_tree_* entry points,
// tdtk_tree_verify and the host builder's layout.
#include "api_internal.h"

using namespace tdtk;

namespace tdtk {

// blocks an enqueued kernel still reads: given back behind the next synchronisation of the context's stream
static void pool_free_later(Ctx* c, void* p) { if (p) c->free_later.push_back(p); }
static void flush_free_later(Ctx* c)
{
  for (void* p : c->free_later) pool_free(p);
  c->free_later.clear();
}

// ---- tree ------------------------------------------------------------------------------
// device construction (build.hip) over the [M][3] points already sitting in c->ws[WS_TMPA]
int tree_from_device_points(Ctx* c, tdtk_tree* t, size_t M, int bucket_size, double t0)
{
  int rc;
  if ((rc = c->ws[WS_BOX].ensure(bbox_temp_bytes() + 8 * sizeof(double)))) return rc;
  double* d_box = c->ws[WS_BOX].as<double>();
  // root bounding box (binning of unsorted query batches, accumulation shift): min / max on the device, and behind them
  // whether a coordinate is a NaN or an infinity.  The build refuses such a cloud only where a split leaves a side empty
  // (children_of, build.hip): a cloud that never splits (M <= bucket) or a single +inf (the mean is +inf, every other point
  // goes left) would get a tree, and a list of the k-nearest walks over it could mix NaN and finite distances, which their
  // "first nr slots" extraction excludes.  So the answer is read here, in front of the build, as kd_build.cpp does
  HIPCHK(launch_bbox(c->ws[WS_TMPA].as<double>(), M, d_box + 8, d_box, c->stream, d_box + 6));
  HIPCHK(hipMemcpyAsync(c->h_pin + Ctx::PIN_BOX, d_box, 7 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->h_pin[Ctx::PIN_BOX + 6] != 0.0) {
    set_error("degenerate split (non-finite coordinates?)");
    return TDTK_EINVAL;
  }
  const double t1 = now_ms();
  t->info.upload_ms = t1 - t0;
  const bool alone = g_ctx_live.load() <= 2;
  if ((rc = c->ws[WS_ARENA].ensure(device_build_arena_bytes(M, alone)))) return rc;
  // The background chain of the build needs a stream of its own, and the runtime has four hardware queues for all the
  // streams of the process: when several host threads are at work -- a doICP that prepares
  // three scans ahead -- a sixth and seventh stream end up queued behind other threads' kernels, the root's chain (one
  // wave, 1.2 ms) in front of somebody's search, and ten 1M-point scans take 43.5 ms instead of 36.4.  So: beside at
  // most one other thread.
  if (alone && !c->stream_b) {
    // made when first needed: every stream of the process takes a share of the four hardware queues, used or not, and
    // the worker threads of a prefetch pool never build alone
    HIPCHK(hipStreamCreateWithFlags(&c->stream_b, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->stream_c, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->stream_d, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->e_b1, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->e_b2, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->e_b3, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->e_b4, hipEventDisableTiming));
  }
  const bool four = [] { const char* e = lab_env("TDTK_BUILD_STREAMS"); return !(e && e[0] == '3'); }();   // (lab: TDTK_BUILD_STREAMS=3: round 5's two side streams)
  const BuildSide side = {alone ? c->stream_b : nullptr, alone ? c->stream_c : nullptr, c->e_b1, c->e_b2, c->e_b3, c->h_build,
                          (alone && four) ? c->stream_d : nullptr, c->e_b4};
  DevBuildResult r = device_build_tree(c->ws[WS_TMPA].as<double>(), M, bucket_size, c->ws[WS_ARENA].p, c->stream, &side);
  if (r.respeculated) g_respeculated.fetch_add(1);
  if (r.err != hipSuccess) {
    set_error(r.degenerate ? std::string("degenerate split (non-finite coordinates?)")
                           : std::string("device tree build: ") + hipGetErrorString(r.err));
    return r.degenerate ? TDTK_EINVAL : TDTK_EDEVICE;
  }
  for (int a = 0; a < 3; a++) { t->bbmin[a] = c->h_pin[Ctx::PIN_BOX + a]; t->bbmax[a] = c->h_pin[Ctx::PIN_BOX + 3 + a]; }
  t->d_nodes = r.nodes; t->d_r = r.node_r; t->d_pts = r.pts;
  t->d_leaf = r.leaf_tab;   // non-null only in table mode
  t->dev.root_ref = r.root_ref;
  t->dev.cb = (uint32_t)r.cb;
  t->info.n_internal = r.n_internal; t->info.n_leaves = r.n_leaves;
  t->info.max_depth = r.max_depth; t->info.max_leaf_points = r.max_leaf;
  std::memcpy(t->build_path, &r.path, sizeof t->build_path);
  t->info.build_ms = now_ms() - t1;
  c->last_build_ms = t->info.build_ms;
  return TDTK_OK;
}

// Pad every bucket to whole groups of four slots and build the fp32 shadow groups the big-batch search filters buckets
// with (kernels.hip, "bucket groups").  The build's scratch arena is free again at this point and holds the two counter
// arrays and the scan's temporary.  Skipped (the tree stays as built, the search scans buckets in fp64 only) when the
// tree is a single bucket, when the padded positions would not fit the reference format, or with TDTK_BUCKET_GROUPS=0.
static int tree_pad_buckets(Ctx* c, tdtk_tree* t, size_t M)
{
  t->Mp = M;
  static const bool off = [] { const char* e = getenv("TDTK_BUCKET_GROUPS"); return e && e[0] == '0'; }();
  if (off || t->info.n_internal == 0) return TDTK_OK;
  const size_t n1 = M + 1;
  const size_t tmpb = scan_u32_temp_bytes(n1);
  const size_t need = 2 * n1 * sizeof(uint32_t) + tmpb + 256;
  int rc;
  if ((rc = c->ws[WS_ARENA].ensure(need))) return rc;
  uint32_t* ng_at = c->ws[WS_ARENA].as<uint32_t>();
  uint32_t* g_at = ng_at + n1;
  void* tmp = (void*)(((uintptr_t)(g_at + n1) + 127) & ~(uintptr_t)127);
  const uint32_t cb = t->dev.cb, cmask = (cb >= 32) ? 0xFFFFFFFFu : ((1u << cb) - 1u);
  KdNode* nodes = static_cast<KdNode*>(t->d_nodes);
  LeafEntry* leaf = static_cast<LeafEntry*>(t->d_leaf);
  HIPCHK(launch_pad_mark(nodes, t->info.n_internal, leaf, cb, cmask, ng_at, M, c->stream));
  HIPCHK(launch_scan_u32(ng_at, g_at, n1, tmp, tmpb, c->stream));
  // The number of groups is known on the device; every bucket is padded by at most three slots, so (M + 3 leaves) / 4 groups
  // are enough room.  When that bound passes the format checks below, the fill is enqueued right away and the exact count is
  // read with it -- one look at the device less (a small scan's tree is a few dozen microseconds of launches per look).
  // the 16-bit grid over the root box (TreeDev::q16): one cell size for the three axes, so that distances stay isotropic
  bool want_q16 = false;
  {
    static const bool q_off = [] { const char* e = getenv("TDTK_BUCKET_Q16"); return e && e[0] == '0'; }();
    double ext = 0.0;
    for (int a = 0; a < 3; a++) ext = std::max(ext, t->bbmax[a] - t->bbmin[a]);
    const double sc = 65535.0 / ext;
    if (!q_off && ext > 0.0 && std::isfinite(ext) && std::isfinite(sc) && sc > 0.0) {
      want_q16 = true;
      for (int a = 0; a < 3; a++) t->q_lo[a] = t->bbmin[a];
      t->q_scale = sc;
    }
  }
  uint32_t G = 0;
  const uint64_t G_bound = ((uint64_t)M + 3ull * t->info.n_leaves + 3ull) / 4ull;
  const bool bound_ok = (4ull * G_bound) * sizeof(KdPoint) < (1ull << 32) && (leaf || ((4ull * G_bound) << cb) <= (uint64_t)REF_VAL);
  if (bound_ok) {
    void *ptsB = nullptr, *grpB = nullptr;
    if (handle_malloc(&ptsB, 4ull * G_bound * sizeof(KdPoint)) == hipSuccess && handle_malloc(&grpB, (size_t)G_bound * 48) == hipSuccess) {
      void* q16B = nullptr;      // (no room for it: the fp32 groups alone)
      if (want_q16 && handle_malloc(&q16B, (size_t)G_bound * 24 + 128) != hipSuccess) { (void)hipGetLastError(); q16B = nullptr; }
      hipError_t e = launch_pad_fill(nodes, t->info.n_internal, leaf, cb, cmask, g_at, static_cast<const KdPoint*>(t->d_pts),
                                     static_cast<KdPoint*>(ptsB), static_cast<float4*>(grpB), c->stream, static_cast<uint32_t*>(q16B), t->q_lo, t->q_scale);
      if (e == hipSuccess) e = hipMemcpyAsync(c->h_pin + Ctx::PIN_GROUPS, g_at + M, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
      if (e != hipSuccess) { pool_free(ptsB); pool_free(grpB); if (q16B) pool_free(q16B); set_error(std::string("bucket groups: ") + hipGetErrorString(e)); return TDTK_EDEVICE; }
      pool_free_later(c, t->d_pts);
      t->d_pts = ptsB; t->d_grp = grpB; t->d_q16 = q16B;
      t->Mp = 0;                 // = 4 G, read in tree_finish behind its synchronisation
      return TDTK_OK;
    }
    (void)hipGetLastError();
    if (ptsB) pool_free(ptsB);
  }
  HIPCHK(hipMemcpyAsync(&G, g_at + M, sizeof G, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const uint64_t slots = 4ull * G;
  // the padded starts must fit where the starts fitted: 30-bit packed references (start << cb | count), 32-bit byte
  // offsets into the point and group arrays, int32 starts of the leaf table
  if (G == 0 || slots * sizeof(KdPoint) >= (1ull << 32) || (!leaf && (slots << cb) > (uint64_t)REF_VAL)) return TDTK_OK;
  // No room for the padded copy (a transient peak of twice the point array + 12 bytes per slot): the tree as it stands is
  // complete and searchable -- nothing has been rewritten yet --, so padding is skipped and the fp64-only bucket scan used.
  void *ptsP = nullptr, *grp = nullptr;
  if (handle_malloc(&ptsP, slots * sizeof(KdPoint)) != hipSuccess) { (void)hipGetLastError(); return TDTK_OK; }
  if (handle_malloc(&grp, (size_t)G * 48) != hipSuccess) { (void)hipGetLastError(); pool_free(ptsP); return TDTK_OK; }
  void* q16 = nullptr;
  if (want_q16 && handle_malloc(&q16, (size_t)G * 24 + 128) != hipSuccess) { (void)hipGetLastError(); q16 = nullptr; }
  hipError_t e = launch_pad_fill(nodes, t->info.n_internal, leaf, cb, cmask, g_at, static_cast<const KdPoint*>(t->d_pts),
                                 static_cast<KdPoint*>(ptsP), static_cast<float4*>(grp), c->stream, static_cast<uint32_t*>(q16), t->q_lo, t->q_scale);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { pool_free(ptsP); pool_free(grp); if (q16) pool_free(q16); set_error(std::string("bucket groups: ") + hipGetErrorString(e)); return TDTK_EDEVICE; }
  pool_free(t->d_pts);
  t->d_pts = ptsP; t->d_grp = grp; t->d_q16 = q16; t->Mp = (size_t)slots;
  return TDTK_OK;
}

int tree_finish(Ctx* c, tdtk_tree* t, size_t M)
{
  int prc = tree_pad_buckets(c, t, M);
  if (prc) return prc;
  for (int a = 0; a < 3; a++) t->centre[a] = 0.5 * (t->bbmin[a] + t->bbmax[a]);
  // the compact hot records (fp32 box + split value + children) the big-batch search kernel walks
  double am = 0.0;
  for (int a = 0; a < 3; a++) am = std::max(am, std::max(std::fabs(t->bbmin[a]), std::fabs(t->bbmax[a])));
  t->dev.absmax = (float)std::min(am * 1.0000002, 3.0e38);
  if (t->info.n_internal) {
    // (+ the split halves on their own behind them, 16 bytes per node, for the visits that defer the quick check: ONE allocation,
    // so that a lane picks between the two by an offset from the same base)
    HIPCHK(handle_malloc(&t->d_hot, t->info.n_internal * (sizeof(KdHot) + sizeof(double2))));
    t->d_split = static_cast<char*>(t->d_hot) + t->info.n_internal * sizeof(KdHot);
    HIPCHK(launch_make_hot(static_cast<const KdNode*>(t->d_nodes), t->info.n_internal, static_cast<KdHot*>(t->d_hot), c->stream,
                           static_cast<double2*>(t->d_split)));
#ifdef TDTK_LAB
    // ... and, on request only, the two-level records (a node with its children's hot parts): two tree levels per round
    // trip are a measured negative both for the persistent-lane kernel (TDTK_FAT_NODES=1) and for the lane-group kernels of
    // small batches (TDTK_FAT_SMALL=1); kernels.hip has the numbers
    static const bool want_fat = [] {
      const char *a = lab_env("TDTK_FAT_NODES"), *b = lab_env("TDTK_FAT_SMALL");
      return (a && a[0] == '1') || (b && b[0] == '1');
    }();
    if (want_fat) {
      HIPCHK(handle_malloc(&t->d_fat, t->info.n_internal * sizeof(KdFat)));
      HIPCHK(launch_make_fat(static_cast<const KdNode*>(t->d_nodes), t->info.n_internal, static_cast<KdFat*>(t->d_fat), c->stream));
    }
#endif
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  if (t->d_grp && t->Mp == 0) {        // the padded layout was filled without a look of its own: its size now
    if (!t->info.n_internal) HIPCHK(hipStreamSynchronize(c->stream));
    uint32_t G = 0;
    std::memcpy(&G, c->h_pin + Ctx::PIN_GROUPS, sizeof G);
    t->Mp = 4ull * G;
  }
  flush_free_later(c);
  t->dev.hot = static_cast<const KdHot*>(t->d_hot);
  t->dev.n_hot = (uint32_t)t->info.n_internal;
  t->dev.n_slots = (uint32_t)std::min<size_t>(t->Mp, 0xFFFFFFFFu);
  t->dev.fat = static_cast<const KdFat*>(t->d_fat);
  t->dev.nodes = static_cast<const KdNode*>(t->d_nodes);
  t->dev.pts = static_cast<const KdPoint*>(t->d_pts);
  t->dev.grp = static_cast<const float4*>(t->d_grp);
  t->dev.q16 = static_cast<const uint32_t*>(t->d_q16);
  t->dev.split = static_cast<const double2*>(t->d_split);
  for (int a = 0; a < 3; a++) t->dev.q_lo[a] = t->q_lo[a];
  t->dev.q_scale = t->q_scale;
  t->dev.leaf_tab = static_cast<const LeafEntry*>(t->d_leaf);
  t->dev.node_r = static_cast<const double*>(t->d_r);
  t->dev.cmask = (t->dev.cb >= 32) ? 0xFFFFFFFFu : ((1u << t->dev.cb) - 1u);
  t->info.n_points = M;
  t->info.device_bytes = t->info.n_internal * (sizeof(KdNode) + sizeof(KdHot) + sizeof(double2) + (t->d_fat ? sizeof(KdFat) : 0) + sizeof(double)) + t->Mp * sizeof(KdPoint) +
                         (t->d_grp ? t->Mp / 4 * 48 : 0) + (t->d_q16 ? t->Mp / 4 * 24 + 128 : 0) +
                         (t->d_leaf ? t->info.n_leaves * sizeof(LeafEntry) : 0);
  return TDTK_OK;
}

int tree_check_args(size_t M, int bucket_size)
{
  if (bucket_size < 1) { set_error("bucket size must be >= 1"); return TDTK_EINVAL; }
  if (M > (size_t)REF_VAL || M * sizeof(KdPoint) >= (1ull << 32)) {
    set_error("model scan too large (30-bit references / 32-bit byte offsets: < 2^27 points)");
    return TDTK_EINVAL;
  }
  return TDTK_OK;
}

}  // namespace tdtk

extern "C" {

int tdtk_tree_create(const double* xyz, size_t M, int bucket_size, int device, tdtk_tree** out)
{
  if (!out) { set_error("out is NULL"); return TDTK_EINVAL; }
  *out = nullptr;
  if (!xyz || M == 0) { set_error("cannot create kdtree with zero points"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(device, &c);
  if (rc) return rc;

  const double t0 = now_ms();
  std::unique_ptr<tdtk_tree> t(new tdtk_tree);
  t->device = device; t->M = M; t->bucket = bucket_size;
  if ((rc = tree_check_args(M, bucket_size))) return rc;
  // device construction (build.hip): upload the points once, build level by level.  (The host builder, kd_build.cpp,
  // is reachable through tdtk_tree_verify only -- it is the cross-check of this path, not an alternative to it.)
  if ((rc = c->ws[WS_TMPA].ensure(3 * M * sizeof(double)))) return rc;
  HIPCHK(hipMemcpyAsync(c->ws[WS_TMPA].p, xyz, 3 * M * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = tree_from_device_points(c, t.get(), M, bucket_size, t0))) return rc;
  if ((rc = tree_finish(c, t.get(), M))) return rc;
  *out = t.release();
  return TDTK_OK;
}

// KDtree over the points of a resident scan as they are now, in the caller's order -- what BasicScan builds
// over "xyz reduced original" (basicScan.cc:702-728) when it is called before the scan has been moved: no trip
// of the points through the host.
int tdtk_tree_create_from_scan(const tdtk_scan* scan, int bucket_size, tdtk_tree** out)
{
  if (!out) { set_error("out is NULL"); return TDTK_EINVAL; }
  *out = nullptr;
  if (!scan || scan->N == 0) { set_error("cannot create kdtree with zero points"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(scan->device, &c);
  if (rc) return rc;
  const double t0 = now_ms();
  const size_t M = scan->N;
  std::unique_ptr<tdtk_tree> t(new tdtk_tree);
  t->device = scan->device; t->M = M; t->bucket = bucket_size;
  if ((rc = tree_check_args(M, bucket_size))) return rc;
  if ((rc = c->ws[WS_TMPA].ensure(3 * M * sizeof(double)))) return rc;
  const bool saved = scan->ox != nullptr;   // moved since tdtk_scan_mark_original: the saved points are the original
  if (!saved && (rc = scan_settle(c, scan))) return rc;
  HIPCHK(launch_unsort_aos(saved ? scan->ox : scan->x, saved ? scan->oy : scan->y, saved ? scan->oz : scan->z,
                           scan->d_order, M, c->ws[WS_TMPA].as<double>(), c->stream));
  if ((rc = tree_from_device_points(c, t.get(), M, bucket_size, t0))) return rc;
  if ((rc = tree_finish(c, t.get(), M))) return rc;
  *out = t.release();
  return TDTK_OK;
}

// KDtreeMetaManaged (src/slam6d/kdMeta.cc:34-134): one tree over the CURRENT points of several resident scans,
// concatenated in the order given, each scan in its caller's order (prepareTempIndices, kdMeta.cc:60-79)
int tdtk_tree_create_from_scans(tdtk_scan* const* scans, int nscans, int bucket_size, tdtk_tree** out)
{
  if (!out) { set_error("out is NULL"); return TDTK_EINVAL; }
  *out = nullptr;
  if (!scans || nscans <= 0 || !scans[0]) { set_error("cannot create kdtree with zero points"); return TDTK_EINVAL; }
  size_t M = 0;
  for (int i = 0; i < nscans; i++) {
    if (!scans[i]) { set_error("NULL scan"); return TDTK_EINVAL; }
    if (scans[i]->device != scans[0]->device) { set_error("scans live on different devices"); return TDTK_EINVAL; }
    M += scans[i]->N;
  }
  if (M == 0) { set_error("cannot create kdtree with zero points"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(scans[0]->device, &c);
  if (rc) return rc;
  const double t0 = now_ms();
  std::unique_ptr<tdtk_tree> t(new tdtk_tree);
  t->device = scans[0]->device; t->M = M; t->bucket = bucket_size;
  if ((rc = tree_check_args(M, bucket_size))) return rc;
  if ((rc = c->ws[WS_TMPA].ensure(3 * M * sizeof(double)))) return rc;
  if ((rc = scans_settle(c, scans, nscans))) return rc;
  size_t off = 0;
  for (int i = 0; i < nscans; i++) {
    const tdtk_scan* sc = scans[i];
    HIPCHK(launch_unsort_aos(sc->x, sc->y, sc->z, sc->d_order, sc->N, c->ws[WS_TMPA].as<double>() + 3 * off, c->stream));
    off += sc->N;
  }
  if ((rc = tree_from_device_points(c, t.get(), M, bucket_size, t0))) return rc;
  if ((rc = tree_finish(c, t.get(), M))) return rc;
  *out = t.release();
  return TDTK_OK;
}

void tdtk_tree_destroy(tdtk_tree* t)
{
  if (!t) return;
  // a batch of scan moves / link passes left running behind the fence may still read this tree: explicit wait, not
  // hipFree's implicit device synchronisation
  wait_deferred(t->device);
  delete t;   // ~tdtk_tree releases the device arrays
}

int tdtk_tree_get_info(const tdtk_tree* t, tdtk_tree_info* info)
{
  if (!t || !info) { set_error("NULL argument"); return TDTK_EINVAL; }
  *info = t->info;
  return TDTK_OK;
}

// ---- diagnostics: which way through the hand-over decisions did the build of this tree take? -----
int tdtk_tree_build_path(const tdtk_tree* t, uint32_t out[12])
{
  if (!t || !out) { set_error("NULL argument"); return TDTK_EINVAL; }
  std::memcpy(out, t->build_path, sizeof t->build_path);
  return TDTK_OK;
}

// ---- diagnostics: is the resident tree bit-identical to the host builder's? ----------------------
int tdtk_tree_verify(const tdtk_tree* t, uint64_t mismatches[4])
{
  if (!t || !mismatches) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(t->device, &c);
  if (rc) return rc;
  // The resident arrays, with the padding of the buckets to whole groups (tree_pad_buckets) undone: the leaves in the
  // order of their (padded) starts give back the packed array and the references the builder emitted.
  std::vector<KdPoint> padded(t->Mp);
  HIPCHK(hipMemcpy(padded.data(), t->d_pts, padded.size() * sizeof(KdPoint), hipMemcpyDeviceToHost));
  std::vector<KdNode> dn(t->info.n_internal);
  std::vector<LeafEntry> dl;
  if (!dn.empty()) HIPCHK(hipMemcpy(dn.data(), t->d_nodes, dn.size() * sizeof(KdNode), hipMemcpyDeviceToHost));
  if (t->d_leaf) { dl.resize(t->info.n_leaves); HIPCHK(hipMemcpy(dl.data(), t->d_leaf, dl.size() * sizeof(LeafEntry), hipMemcpyDeviceToHost)); }
  std::vector<KdPoint> pts;
  uint64_t group_errors = 0;
  // the search-side copies of a node's split half (the hot record's, and the 16-byte one the deferred quick check reads) say
  // what the node says
  if (t->d_hot && !dn.empty()) {
    std::vector<KdHot> hot(dn.size());
    HIPCHK(hipMemcpy(hot.data(), t->d_hot, hot.size() * sizeof(KdHot), hipMemcpyDeviceToHost));
    struct Half { double splitval; uint32_t c1, c2; };
    std::vector<Half> half;
    if (t->d_split) { half.resize(dn.size()); HIPCHK(hipMemcpy(half.data(), t->d_split, half.size() * sizeof(Half), hipMemcpyDeviceToHost)); }
    for (size_t i = 0; i < dn.size(); i++) {
      if (std::memcmp(&hot[i].splitval, &dn[i].splitval, 8) != 0 || hot[i].c1 != dn[i].c1 || hot[i].c2 != dn[i].c2) group_errors++;
      if (!half.empty() && (std::memcmp(&half[i].splitval, &dn[i].splitval, 8) != 0 || half[i].c1 != dn[i].c1 || half[i].c2 != dn[i].c2)) group_errors++;
    }
  }
  if (t->d_grp) {
    const uint32_t cbv = t->dev.cb, cm = (cbv >= 32) ? 0xFFFFFFFFu : ((1u << cbv) - 1u);
    struct Run { uint32_t start, count; uint32_t* ref; LeafEntry* le; };
    std::vector<Run> runs;
    for (KdNode& nd : dn)
      for (uint32_t* r : {&nd.c1, &nd.c2})
        if (*r & REF_LEAF) {
          const uint32_t v = *r & REF_VAL;
          if (t->d_leaf) runs.push_back({(uint32_t)dl[v].start, (uint32_t)dl[v].count, nullptr, &dl[v]});
          else runs.push_back({v >> cbv, v & cm, r, nullptr});
        }
    std::sort(runs.begin(), runs.end(), [](const Run& a, const Run& b) { return a.start < b.start; });
    std::vector<float> shadow((size_t)t->Mp * 3);
    HIPCHK(hipMemcpy(shadow.data(), t->d_grp, shadow.size() * sizeof(float), hipMemcpyDeviceToHost));
    // the 16-bit shadow (TreeDev::q16): every slot's grid indices recomputed here with the grid the tree carries
    std::vector<uint16_t> q16;
    if (t->d_q16) {
      q16.resize((size_t)t->Mp * 3);
      HIPCHK(hipMemcpy(q16.data(), t->d_q16, q16.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    }
    auto grid_index = [&](double v, int a) -> uint16_t {       // kernels.hip: q16_index
      const double u = (v - t->q_lo[a]) * t->q_scale + 0.5;
      int i = (!(u >= 0.0)) ? -32768 : ((!(u < 65536.0)) ? 32767 : (int)u - 32768);
      return (uint16_t)(i & 0xFFFF);
    };
    pts.reserve(t->M);
    uint32_t expect = 0;
    for (const Run& r : runs) {
      if (r.start != expect || (r.start & 3u) || r.count == 0 || (size_t)r.start + r.count > t->Mp) { group_errors++; break; }
      const uint32_t packed = (uint32_t)pts.size(), ng = (r.count + 3u) >> 2;
      for (uint32_t j = 0; j < 4 * ng; j++) {
        const KdPoint& P = padded[r.start + j];
        const KdPoint& L = padded[r.start + std::min(j, r.count - 1)];
        if (j < r.count) pts.push_back(P);
        else if (std::memcmp(&P, &L, sizeof P) != 0) group_errors++;     // a pad slot repeats the bucket's last point
        const size_t g = (r.start + j) >> 2, k = j & 3u;
        if (shadow[g * 12 + k] != (float)L.x || shadow[g * 12 + 4 + k] != (float)L.y || shadow[g * 12 + 8 + k] != (float)L.z) group_errors++;
        if (!q16.empty()) {
          // two slots per 12 bytes: { (x0, y0), (x1, y1), (z0, z1) } as six uint16
          const size_t pr = (size_t)(r.start + j) >> 1, hi = (r.start + j) & 1u;
          const uint16_t* w = &q16[pr * 6];
          if (w[2 * hi] != grid_index(L.x, 0) || w[2 * hi + 1] != grid_index(L.y, 1) || w[4 + hi] != grid_index(L.z, 2)) group_errors++;
        }
      }
      expect = r.start + 4 * ng;
      if (r.le) r.le->start = (int32_t)packed;
      else *r.ref = (*r.ref & ~REF_VAL) | (packed << cbv) | r.count;
    }
    if (expect != t->Mp || pts.size() != t->M) group_errors++;
    if (group_errors) { mismatches[0] = mismatches[1] = mismatches[2] = 0; mismatches[3] = group_errors; return TDTK_OK; }
  } else {
    pts = padded;
    if (group_errors) { mismatches[0] = mismatches[1] = mismatches[2] = 0; mismatches[3] = group_errors; return TDTK_OK; }
  }
  // recover the caller's array from the resident points (each carries its caller index)
  std::vector<double> xyz(3 * t->M);
  for (size_t k = 0; k < t->M; k++) {
    const size_t o = (size_t)pts[k].orig;
    if (o >= t->M) { mismatches[0] = mismatches[1] = mismatches[2] = 0; mismatches[3] = 1; return TDTK_OK; }
    xyz[3 * o] = pts[k].x; xyz[3 * o + 1] = pts[k].y; xyz[3 * o + 2] = pts[k].z;
  }
  HostTree H;
  std::string err;
  if (!build_tree(xyz.data(), t->M, t->bucket, H, err)) { set_error(err); return TDTK_EINVAL; }
  std::vector<KdNode> nodes(H.nodes.size());
  std::vector<double> rr(H.nodes.size());
  mismatches[0] = mismatches[1] = mismatches[2] = mismatches[3] = 0;
  if (H.n_internal != t->info.n_internal || H.n_leaves != t->info.n_leaves || H.max_depth != t->info.max_depth ||
      H.max_leaf_points != t->info.max_leaf_points || H.root_ref != t->dev.root_ref || (uint32_t)H.cb != t->dev.cb ||
      H.table_mode != (t->d_leaf != nullptr))
    mismatches[3] = 1;
  if (mismatches[3] == 0) {
    if (!nodes.empty()) {
      nodes = dn;    // with the references pointing into the packed array again
      HIPCHK(hipMemcpy(rr.data(), t->d_r, rr.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < nodes.size(); i++) {
      const KdNode &a = nodes[i], &b = H.nodes[i];
      // == on doubles: +0 and -0 compare equal (the sign of a zero box centre never decides anything)
      if (!(a.cx == b.cx && a.cy == b.cy && a.cz == b.cz && a.hx == b.hx && a.hy == b.hy && a.hz == b.hz &&
            a.splitval == b.splitval && a.c1 == b.c1 && a.c2 == b.c2)) {
        mismatches[0]++;
        if (kLab && lab_env("TDTK_VERIFY_DUMP"))
          fprintf(stderr, "VERIFY node %zu: dev c(%.17g %.17g %.17g) h(%.17g %.17g %.17g) split %.17g c1 %08x c2 %08x\n"
                          "            host c(%.17g %.17g %.17g) h(%.17g %.17g %.17g) split %.17g c1 %08x c2 %08x\n",
                  i, a.cx, a.cy, a.cz, a.hx, a.hy, a.hz, a.splitval, a.c1, a.c2, b.cx, b.cy, b.cz, b.hx, b.hy, b.hz, b.splitval, b.c1, b.c2);
      }
      if (rr[i] != H.node_r[i]) mismatches[1]++;
    }
    for (size_t i = 0; i < pts.size(); i++)
      if (!(pts[i].x == H.pts[i].x && pts[i].y == H.pts[i].y && pts[i].z == H.pts[i].z && pts[i].orig == H.pts[i].orig))
        mismatches[2]++;
    if (H.table_mode) {
      std::vector<LeafEntry> lt = dl;
      // leaf ids may be numbered differently; compare through the references instead
      auto leaf_of = [&](const std::vector<LeafEntry>& tab, uint32_t ref) { return tab[ref & REF_VAL]; };
      for (size_t i = 0; i < nodes.size(); i++)
        for (int k = 0; k < 2; k++) {
          const uint32_t ra = k ? nodes[i].c2 : nodes[i].c1, rb = k ? H.nodes[i].c2 : H.nodes[i].c1;
          if ((ra & REF_LEAF) != (rb & REF_LEAF)) continue;
          if (ra & REF_LEAF) {
            const LeafEntry x = leaf_of(lt, ra), y = leaf_of(H.leaf_tab, rb);
            if (x.start != y.start || x.count != y.count) mismatches[3]++;
          }
        }
    }
  }
  return TDTK_OK;
}

// ---- host-only diagnostics -----------------------------------------------------------------
int tdtk_host_tree_layout(const double* xyz, size_t M, int bucket_size, int32_t* perm_out, uint64_t stats[4])
{
  HostTree H;
  std::string err;
  if (!build_tree(xyz, M, bucket_size, H, err)) { set_error(err); return TDTK_EINVAL; }
  if (perm_out)
    for (size_t k = 0; k < M; k++) perm_out[k] = H.pts[k].orig;
  if (stats) { stats[0] = H.n_internal; stats[1] = H.n_leaves; stats[2] = H.max_depth; stats[3] = H.max_leaf_points; }
  return TDTK_OK;
}

// The level profile of the host builder's tree: per depth how many nodes (internal and buckets) it has and how many points
// the largest of them holds -- what the device build's looks see (k_fin_maxn) when its tree is the host builder's.
// nseg / maxn hold `cap` entries (deeper levels are counted in *levels only).
int tdtk_host_tree_levels(const double* xyz, size_t M, int bucket_size, int cap, uint32_t* nseg, uint32_t* maxn, int* levels)
{
  if (!nseg || !maxn || !levels || cap < 0) { set_error("NULL argument"); return TDTK_EINVAL; }
  HostTree H;
  std::string err;
  if (!build_tree(xyz, M, bucket_size, H, err)) { set_error(err); return TDTK_EINVAL; }
  const uint32_t cmask = (H.cb >= 32) ? 0xFFFFFFFFu : ((1u << H.cb) - 1u);
  auto bucket_points = [&](uint32_t ref) -> uint32_t {
    return H.table_mode ? (uint32_t)H.leaf_tab[ref & REF_VAL].count : ((ref & REF_VAL) & cmask);
  };
  const size_t n = H.nodes.size();
  // subtree sizes bottom-up: in breadth-first order a node's children come behind it
  std::vector<uint32_t> size(n), depth(n);
  auto points_of = [&](uint32_t ref) -> uint32_t { return (ref & REF_LEAF) ? bucket_points(ref) : size[ref & REF_VAL]; };
  for (size_t i = n; i-- > 0;) size[i] = points_of(H.nodes[i].c1) + points_of(H.nodes[i].c2);
  std::fill(nseg, nseg + cap, 0u);
  std::fill(maxn, maxn + cap, 0u);
  uint32_t deepest = 0;
  auto count = [&](uint32_t d, uint32_t points) {
    deepest = std::max(deepest, d);
    if (d < (uint32_t)cap) { nseg[d]++; maxn[d] = std::max(maxn[d], points); }
  };
  // depths top-down
  count(0u, points_of(H.root_ref));
  for (size_t i = 0; i < n; i++) {
    if (i == 0) depth[0] = 0u;
    for (uint32_t ref : {H.nodes[i].c1, H.nodes[i].c2}) {
      count(depth[i] + 1u, points_of(ref));
      if (!(ref & REF_LEAF)) depth[ref & REF_VAL] = depth[i] + 1u;
    }
  }
  *levels = (int)deepest + 1;
  return TDTK_OK;
}

}  // extern "C"
