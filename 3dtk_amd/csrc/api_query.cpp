// Everything that launches query.hip: k-NN, fixed-radius, cylinder / box / segment queries, collision detection along a
// trajectory, and the normals built on the k-NN and range walks.
#include "api_internal.h"
#include "query.h"

using namespace tdtk;

// ---- k-NN and fixed-radius search (query.hip) ------------------------------------------------
// the K queries at d_q [K][3], spatially binned into WS_QX / WS_QY / WS_QZ (order: sorted position -> caller index), the
// tree's walk arguments and the stack overflow area
// (d_v: a second vector per query [K][3], carried through the bin into WS_DX / WS_DY / WS_DZ -- the cylinder, box and
// segment queries)
// (box: 6 doubles, the lower and upper corner the bin's grid spans instead of the tree's root box; n_walks: the number of
// walks the overflow area is sized for, where that is not K -- the collision kernels bin their model and walk once per
// (frame, model point))
namespace tdtk {
int query_prepare(Ctx* c, const tdtk_tree* t, const double* d_q, size_t K, QueryArgs& a, const double* d_v, const double* box,
                  size_t n_walks)
{
  int rc;
  int ids[] = {WS_QX, WS_QY, WS_QZ};
  for (int id : ids)
    if ((rc = c->ws[id].ensure(K * sizeof(double)))) return rc;
  if (d_v) {
    int vids[] = {WS_DX, WS_DY, WS_DZ};
    for (int id : vids)
      if ((rc = c->ws[id].ensure(K * sizeof(double)))) return rc;
  }
  if ((rc = c->ws[WS_ORDER].ensure(K * sizeof(int32_t)))) return rc;
  if ((rc = c->ws[WS_CELL].ensure(K * sizeof(uint32_t)))) return rc;
  if ((rc = c->ws[WS_HIST].ensure(32768 * sizeof(uint32_t)))) return rc;
  BinArgs b{};
  b.q = d_q; b.dir = d_v; b.n = K;
  for (int ax = 0; ax < 3; ax++) {
    b.lo[ax] = box ? box[ax] : t->bbmin[ax];
    const double ext = (box ? box[3 + ax] : t->bbmax[ax]) - b.lo[ax];
    b.scale[ax] = (ext > 0) ? 32.0 / ext : 0.0;
  }
  b.hist = c->ws[WS_HIST].as<uint32_t>();
  b.cell = c->ws[WS_CELL].as<uint32_t>();
  b.sx = c->ws[WS_QX].as<double>(); b.sy = c->ws[WS_QY].as<double>(); b.sz = c->ws[WS_QZ].as<double>();
  if (d_v) { b.sdx = c->ws[WS_DX].as<double>(); b.sdy = c->ws[WS_DY].as<double>(); b.sdz = c->ws[WS_DZ].as<double>(); }
  b.order = c->ws[WS_ORDER].as<int32_t>();
  HIPCHK(launch_bin(b, c->stream));
  a = QueryArgs{};
  a.node_r = t->dev.node_r; a.vx = b.sdx; a.vy = b.sdy; a.vz = b.sdz;
  a.nodes = t->dev.nodes; a.pts = t->dev.pts; a.leaf_tab = t->dev.leaf_tab;
  a.root_ref = t->dev.root_ref; a.cb = t->dev.cb; a.cmask = t->dev.cmask;
  a.x = b.sx; a.y = b.sy; a.z = b.sz; a.order = b.order; a.n = K;
  const size_t ovf = query_overflow_entries(n_walks ? n_walks : K, t->info.max_depth);
  if (ovf) {
    if ((rc = c->ws[WS_OVF_M2].ensure(ovf * sizeof(double)))) return rc;
    if ((rc = c->ws[WS_OVF_REF].ensure(ovf * sizeof(uint32_t)))) return rc;
    a.ovf_m2 = c->ws[WS_OVF_M2].as<double>();
    a.ovf_ref = c->ws[WS_OVF_REF].as<uint32_t>();
  }
  return TDTK_OK;
}
}  // namespace tdtk

namespace tdtk {
int knn_check_k(int k)
{
  if (k < 1) { set_error("k must be >= 1"); return TDTK_EINVAL; }
  if (k > KNN_MAX_K) { set_error("k = " + std::to_string(k) + " exceeds the supported list capacity of " + std::to_string(KNN_MAX_K)); return TDTK_EUNSUP; }
  return TDTK_OK;
}
}  // namespace tdtk

// a tree over host points [n][3] for the normal estimators; the points stay in WS_TMPA (the build only reads them)
static int normals_tree(Ctx* c, const double* xyz, size_t n, int bucket, int device, std::unique_ptr<tdtk_tree>& t)
{
  int rc;
  t.reset(new tdtk_tree);
  t->device = device; t->M = n; t->bucket = bucket;
  if ((rc = tree_check_args(n, bucket))) return rc;
  if ((rc = c->ws[WS_TMPA].ensure(3 * n * sizeof(double)))) return rc;
  HIPCHK(hipMemcpyAsync(c->ws[WS_TMPA].p, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = tree_from_device_points(c, t.get(), n, bucket, now_ms()))) return rc;
  return tree_finish(c, t.get(), n);
}

// the K queries at q [K][3] uploaded to WS_TMPA -- with v, their second vectors [K][3] side by side behind them -- and
// query_prepare over them
static int query_begin(Ctx* c, const tdtk_tree* t, const double* q, const double* v, size_t K, QueryArgs& a)
{
  int rc;
  if ((rc = c->ws[WS_TMPA].ensure((v ? 6 : 3) * K * sizeof(double)))) return rc;
  double* dq = c->ws[WS_TMPA].as<double>();
  double* dv = v ? dq + 3 * K : nullptr;
  HIPCHK(hipMemcpyAsync(dq, q, 3 * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (v) HIPCHK(hipMemcpyAsync(dv, v, 3 * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return query_prepare(c, t, dq, K, a, dv);
}

// tdtk_kernel_timing(1): HIP events around the count walk of a list query and the link walk of the clustering
static bool walk_timed() { return g_kernel_timing.load(std::memory_order_relaxed) > 0; }

// A list query in two walks over the a.n queries of the prepared block `a` (r2 set): the count walk into WS_KPOS, the scan
// into WS_D2 (WS_ARENA its scratch), the offsets to the host, and, where the caller's capacity holds the total, the fill walk
// into WS_IDX (and WS_TMPB for d2, nullable).  count() and fill() launch the two walks on the context's stream and return a
// TDTK code (the launch's error text is theirs); they read `a` as it stands when they are called.  `noun`: what the capacity
// error counts; timed: HIP events around the count walk (tdtk_last_kernel_ms)
namespace tdtk {
int list_walks(Ctx* c, const char* name, const char* noun, QueryArgs& a, bool timed, const std::function<int()>& count,
               const std::function<int()>& fill, uint64_t* offsets, int32_t* idx, double* d2, size_t cap, uint64_t* total)
{
  int rc;
  hipStream_t s = c->stream;
  const size_t K = a.n;
  const size_t tmpb = range_scan_temp_bytes(K);
  if ((rc = c->ws[WS_KPOS].ensure((K + 1) * sizeof(uint32_t)))) return rc;
  if ((rc = c->ws[WS_D2].ensure((K + 1) * sizeof(unsigned long long)))) return rc;
  if ((rc = c->ws[WS_ARENA].ensure(tmpb + 256))) return rc;
  a.counts = c->ws[WS_KPOS].as<uint32_t>();
  unsigned long long* d_off = c->ws[WS_D2].as<unsigned long long>();
  HIPCHK(hipMemsetAsync(a.counts + K, 0, sizeof(uint32_t), s));
  if (timed) HIPCHK(hipEventRecord(c->e0, s));
  if ((rc = count())) return rc;
  if (timed) { HIPCHK(hipEventRecord(c->e1, s)); c->ev_pending = true; }
  HIPCHK(launch_range_scan(a.counts, d_off, K, c->ws[WS_ARENA].p, tmpb, s));
  HIPCHK(hipMemcpyAsync(offsets, d_off, (K + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const uint64_t tot = offsets[K];
  *total = tot;
  if (cap < tot) {
    set_error(std::string(name) + ": " + std::to_string(tot) + " " + noun + ", capacity " + std::to_string(cap) + " (offsets and total are filled)");
    return TDTK_EINVAL;
  }
  if (tot == 0) return TDTK_OK;
  if (!idx) { set_error("idx is NULL"); return TDTK_EINVAL; }
  if ((rc = c->ws[WS_IDX].ensure(tot * sizeof(int32_t)))) return rc;
  if (d2 && (rc = c->ws[WS_TMPB].ensure(tot * sizeof(double)))) return rc;
  a.offsets = d_off;
  a.idx = c->ws[WS_IDX].as<int32_t>();
  a.d2 = d2 ? c->ws[WS_TMPB].as<double>() : nullptr;
  if ((rc = fill())) return rc;
  HIPCHK(hipMemcpyAsync(idx, a.idx, tot * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (d2) HIPCHK(hipMemcpyAsync(d2, a.d2, tot * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return TDTK_OK;
}
}  // namespace tdtk

// the list queries of a tree: the fixed radius (mode < 0; d2 nullable) and the four shape walks of query.hip (mode: ShapeMode,
// v their second vector)
static int list_query(const char* name, const char* noun, int mode, const tdtk_tree* t, const double* q, const double* v,
                      size_t K, double r2, uint64_t* offsets, int32_t* idx, double* d2, size_t cap, uint64_t* total)
{
  Ctx* c;
  int rc;
  if ((rc = get_ctx(t->device, &c))) return rc;
  offsets[0] = 0; *total = 0;
  if (K == 0) return TDTK_OK;
  hipStream_t s = c->stream;
  QueryArgs a;
  if ((rc = query_begin(c, t, q, v, K, a))) return rc;
  a.r2 = r2;
  auto count = [&]() { HIPCHK(mode < 0 ? launch_range_count(a, s) : launch_shape_count(a, mode, s)); return TDTK_OK; };
  auto fill = [&]() { HIPCHK(mode < 0 ? launch_range_fill(a, s) : launch_shape_fill(a, mode, s)); return TDTK_OK; };
  return list_walks(c, name, noun, a, walk_timed(), count, fill, offsets, idx, d2, cap, total);
}

extern "C" {

int tdtk_knn_search(const tdtk_tree* t, const double* q, size_t K, int k, int32_t* idx, double* d2)
{
  if (!t || (!q && K) || (!idx && K)) { set_error("NULL argument"); return TDTK_EINVAL; }
  int rc;
  if ((rc = knn_check_k(k))) return rc;
  Ctx* c;
  if ((rc = get_ctx(t->device, &c))) return rc;
  if (K == 0) return TDTK_OK;
  const size_t L = K * (size_t)k;
  QueryArgs a;
  if ((rc = query_begin(c, t, q, nullptr, K, a))) return rc;
  if ((rc = c->ws[WS_IDX].ensure(L * sizeof(int32_t)))) return rc;
  if (d2 && (rc = c->ws[WS_TMPB].ensure(L * sizeof(double)))) return rc;
  a.k = k;
  a.idx = c->ws[WS_IDX].as<int32_t>();
  a.d2 = d2 ? c->ws[WS_TMPB].as<double>() : nullptr;
  HIPCHK(launch_knn(a, false, c->stream));
  HIPCHK(hipMemcpyAsync(idx, a.idx, L * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (d2) HIPCHK(hipMemcpyAsync(d2, a.d2, L * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TDTK_OK;
}

int tdtk_knn_range_search(const tdtk_tree* t, const double* q, size_t K, int k, double sqRad2, int32_t* idx, double* d2,
                          int32_t* counts)
{
  if (!t || (!q && K) || (!idx && K)) { set_error("NULL argument"); return TDTK_EINVAL; }
  int rc;
  if ((rc = knn_check_k(k))) return rc;
  if (!std::isfinite(sqRad2)) { set_error("sqRad2 must be finite"); return TDTK_EINVAL; }
  Ctx* c;
  if ((rc = get_ctx(t->device, &c))) return rc;
  if (K == 0) return TDTK_OK;
  const size_t L = K * (size_t)k;
  if (sqRad2 <= 0) {     // no Dist2 is below it: every list is empty, nothing to walk
    std::fill(idx, idx + L, -1);
    if (d2) std::fill(d2, d2 + L, -1.0);
    if (counts) std::fill(counts, counts + K, 0);
    return TDTK_OK;
  }
  QueryArgs a;
  if ((rc = query_begin(c, t, q, nullptr, K, a))) return rc;
  if ((rc = c->ws[WS_IDX].ensure((L + K) * sizeof(int32_t)))) return rc;       // WS_IDX: the lists | counts
  if (d2 && (rc = c->ws[WS_TMPB].ensure(L * sizeof(double)))) return rc;
  a.k = k;
  a.r2 = sqRad2;
  a.idx = c->ws[WS_IDX].as<int32_t>();
  a.d2 = d2 ? c->ws[WS_TMPB].as<double>() : nullptr;
  a.nr_out = counts ? a.idx + L : nullptr;
  HIPCHK(launch_knn_range(a, false, c->stream));
  HIPCHK(hipMemcpyAsync(idx, a.idx, L * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (d2) HIPCHK(hipMemcpyAsync(d2, a.d2, L * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (counts) HIPCHK(hipMemcpyAsync(counts, a.nr_out, K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TDTK_OK;
}

int tdtk_fixed_range_search(const tdtk_tree* t, const double* q, size_t K, double sqRad2, uint64_t* offsets, int32_t* idx,
                            double* d2, size_t cap, uint64_t* total)
{
  if (!t || (!q && K) || !offsets || !total) { set_error("NULL argument"); return TDTK_EINVAL; }
  return list_query("fixedRangeSearch", "neighbours", -1, t, q, nullptr, K, sqRad2, offsets, idx, d2, cap, total);
}

int tdtk_fixed_range_search_along_dir(const tdtk_tree* t, const double* p, const double* dir, size_t K, double maxdist2,
                                      uint64_t* offsets, int32_t* idx, size_t cap, uint64_t* total)
{
  if (!t || ((!p || !dir) && K) || !offsets || !total) { set_error("NULL argument"); return TDTK_EINVAL; }
  return list_query("fixedRangeSearchAlongDir", "points", SHAPE_ALONG_DIR, t, p, dir, K, maxdist2, offsets, idx, nullptr, cap, total);
}

int tdtk_fixed_range_search_between(const tdtk_tree* t, const double* p, const double* p0, size_t K, double maxdist2,
                                    uint64_t* offsets, int32_t* idx, size_t cap, uint64_t* total)
{
  if (!t || ((!p || !p0) && K) || !offsets || !total) { set_error("NULL argument"); return TDTK_EINVAL; }
  return list_query("fixedRangeSearchBetween2Points", "points", SHAPE_BETWEEN, t, p, p0, K, maxdist2, offsets, idx, nullptr, cap, total);
}

int tdtk_aabb_search(const tdtk_tree* t, const double* lo, const double* hi, size_t K, uint64_t* offsets, int32_t* idx,
                     size_t cap, uint64_t* total)
{
  if (!t || ((!lo || !hi) && K) || !offsets || !total) { set_error("NULL argument"); return TDTK_EINVAL; }
  // kdIndexed.cc:237-238, the comparison in the reference's sense (a NaN corner passes it); nothing is written or launched
  for (size_t i = 0; i < 3 * K; i++)
    if (lo[i] > hi[i]) { set_error("invalid bbox"); return TDTK_EINVAL; }
  return list_query("AABBSearch", "points", SHAPE_AABB, t, lo, hi, K, 0.0, offsets, idx, nullptr, cap, total);
}

int tdtk_segment_search_all(const tdtk_tree* t, const double* p, const double* p0, size_t K, double maxdist2,
                            uint64_t* offsets, int32_t* idx, size_t cap, uint64_t* total)
{
  if (!t || ((!p || !p0) && K) || !offsets || !total) { set_error("NULL argument"); return TDTK_EINVAL; }
  return list_query("segmentSearch_all", "points", SHAPE_SEGMENT, t, p, p0, K, maxdist2, offsets, idx, nullptr, cap, total);
}

int tdtk_segment_search_nearest(const tdtk_tree* t, const double* p, const double* p0, size_t K, double maxdist2,
                                int32_t* idx, double* d2)
{
  if (!t || ((!p || !p0 || !idx) && K)) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc;
  if ((rc = get_ctx(t->device, &c))) return rc;
  if (K == 0) return TDTK_OK;
  hipStream_t s = c->stream;
  QueryArgs a;
  if ((rc = query_begin(c, t, p, p0, K, a))) return rc;
  if ((rc = c->ws[WS_IDX].ensure(K * sizeof(int32_t)))) return rc;
  if (d2 && (rc = c->ws[WS_TMPB].ensure(K * sizeof(double)))) return rc;
  a.r2 = maxdist2;
  a.idx = c->ws[WS_IDX].as<int32_t>();
  a.d2 = d2 ? c->ws[WS_TMPB].as<double>() : nullptr;
  HIPCHK(launch_segment_nearest(a, s));
  HIPCHK(hipMemcpyAsync(idx, a.idx, K * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (d2) HIPCHK(hipMemcpyAsync(d2, a.d2, K * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return TDTK_OK;
}

}  // extern "C"

// ---- collision detection along a trajectory (query.hip, "collision detection") ------------------------------------------
// the checks the marking and the axis depth share; F * P items at most
static int collide_check_args(const double* model, size_t P, const double* frames, size_t F, double radius)
{
  if (!model || (!frames && F)) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (P == 0) { set_error("the point model is empty"); return TDTK_EINVAL; }
  if (!std::isfinite(radius) || !(radius > 0)) { set_error("radius must be finite and > 0"); return TDTK_EINVAL; }
  size_t items;
  if (__builtin_mul_overflow(F, P, &items)) { set_error("frames x model points exceeds size_t"); return TDTK_EINVAL; }
  return TDTK_OK;
}

// the model [P][3] and the frames [F][16] side by side in WS_TMPB, the model binned on its own bounding box (a non-finite
// coordinate takes no part in the box and lands in a border cell) into WS_QX / WS_QY / WS_QZ; `items` walks
static int collide_prepare(Ctx* c, const tdtk_tree* t, const double* model, size_t P, const double* frames, size_t F,
                           size_t items, double radius, QueryArgs& a)
{
  int rc;
  if ((rc = c->ws[WS_TMPB].ensure((3 * P + 16 * F) * sizeof(double)))) return rc;
  double* d_model = c->ws[WS_TMPB].as<double>();
  double* d_frames = d_model + 3 * P;
  HIPCHK(hipMemcpyAsync(d_model, model, 3 * P * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (F) HIPCHK(hipMemcpyAsync(d_frames, frames, 16 * F * sizeof(double), hipMemcpyHostToDevice, c->stream));
  double box[6] = {0, 0, 0, 0, 0, 0};
  for (int ax = 0; ax < 3; ax++) {
    bool any = false;
    for (size_t i = 0; i < P; i++) {
      const double v = model[3 * i + ax];
      if (!std::isfinite(v)) continue;
      if (!any || v < box[ax]) box[ax] = v;
      if (!any || v > box[3 + ax]) box[3 + ax] = v;
      any = true;
    }
  }
  if ((rc = query_prepare(c, t, d_model, P, a, nullptr, box, items))) return rc;
  a.order = nullptr;
  a.n = items;
  a.P = P;
  a.frames = d_frames;
  a.r2 = radius * radius;
  return TDTK_OK;
}

// the points of env_xyz [M][3] whose mask byte is (take != 0) or is not (take == 0) set, in ascending index
static std::vector<double> collide_compact(const double* env_xyz, size_t M, const uint8_t* colliding, int take)
{
  std::vector<double> out;
  for (size_t i = 0; i < M; i++)
    if ((colliding[i] != 0) == (take != 0)) out.insert(out.end(), env_xyz + 3 * i, env_xyz + 3 * i + 3);
  return out;
}

extern "C" {

int tdtk_collision_mark(const tdtk_tree* env, const double* model, size_t P, const double* frames, size_t F, double radius,
                        int cmethod, uint8_t* colliding, uint64_t* num_colliding)
{
  if (!env || !colliding || !num_colliding) { set_error("NULL argument"); return TDTK_EINVAL; }
  int rc;
  if ((rc = collide_check_args(model, P, frames, F, radius))) return rc;
  if (cmethod != 1 && cmethod != 2) { set_error("cmethod must be 1 (spheres) or 2 (segments)"); return TDTK_EINVAL; }
  if (cmethod == 2 && F == 0) { set_error("the segment method needs a trajectory of at least one frame"); return TDTK_EINVAL; }
  Ctx* c;
  if ((rc = get_ctx(env->device, &c))) return rc;
  hipStream_t s = c->stream;
  const size_t M = env->M;
  const size_t items = (cmethod == 1 ? F : F - 1) * P;
  // WS_IDX: the count (8 bytes) | the mask
  if ((rc = c->ws[WS_IDX].ensure(8 + M))) return rc;
  unsigned long long* d_count = c->ws[WS_IDX].as<unsigned long long>();
  uint8_t* d_mask = c->ws[WS_IDX].as<uint8_t>() + 8;
  HIPCHK(hipMemsetAsync(c->ws[WS_IDX].p, 0, 8 + M, s));
  if (items) {
    QueryArgs a;
    if ((rc = collide_prepare(c, env, model, P, frames, F, items, radius, a))) return rc;
    a.mask = d_mask;
    HIPCHK(launch_collide_mark(a, cmethod, s));
    HIPCHK(launch_collide_count(d_mask, M, d_count, s));
  }
  unsigned long long count = 0;
  HIPCHK(hipMemcpyAsync(colliding, d_mask, M, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&count, d_count, sizeof(count), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *num_colliding = count;
  return TDTK_OK;
}

int tdtk_collision_depth_closest(const double* env_xyz, size_t M, const uint8_t* colliding, int bucket, int device,
                                 float* dist, uint64_t* n_unreached)
{
  if (!env_xyz || !colliding || !dist) { set_error("NULL argument"); return TDTK_EINVAL; }
  size_t nc = 0;
  for (size_t i = 0; i < M; i++) nc += colliding[i] != 0;
  if (nc == 0) { set_error("no colliding point"); return TDTK_EINVAL; }
  if (nc == M) { set_error("no non-colliding point (the tree would be empty)"); return TDTK_EINVAL; }
  int rc;
  if ((rc = tree_check_args(M - nc, bucket))) return rc;
  Ctx* c;
  if ((rc = get_ctx(device, &c))) return rc;
  const std::vector<double> rest = collide_compact(env_xyz, M, colliding, 0);
  const std::vector<double> hit = collide_compact(env_xyz, M, colliding, 1);
  std::unique_ptr<tdtk_tree> t;
  if ((rc = normals_tree(c, rest.data(), M - nc, bucket, device, t))) return rc;
  std::vector<int32_t> idx(nc);
  std::vector<double> d2(nc);
  if ((rc = tdtk_find_closest(t.get(), hit.data(), nc, 1000000.0, idx.data(), d2.data()))) return rc;
  uint64_t unreached = 0;
  for (size_t i = 0; i < nc; i++) {
    if (idx[i] < 0) { dist[i] = 1000.0f; ++unreached; }
    else dist[i] = (float)std::sqrt(d2[i]);
  }
  if (n_unreached) *n_unreached = unreached;
  return TDTK_OK;
}

int tdtk_collision_depth_axis(const double* env_xyz, size_t M, const uint8_t* colliding, const double* model, size_t P,
                              const double* frames, size_t F, double radius, int bucket, int device, float* dist)
{
  if (!env_xyz || !colliding || !dist) { set_error("NULL argument"); return TDTK_EINVAL; }
  int rc;
  if ((rc = collide_check_args(model, P, frames, F, radius))) return rc;
  size_t nc = 0;
  for (size_t i = 0; i < M; i++) nc += colliding[i] != 0;
  if (nc == 0) { set_error("no colliding point (the tree would be empty)"); return TDTK_EINVAL; }
  if ((rc = tree_check_args(nc, bucket))) return rc;
  Ctx* c;
  if ((rc = get_ctx(device, &c))) return rc;
  hipStream_t s = c->stream;
  const std::vector<double> hit = collide_compact(env_xyz, M, colliding, 1);
  std::unique_ptr<tdtk_tree> t;
  if ((rc = normals_tree(c, hit.data(), nc, bucket, device, t))) return rc;
  // WS_D2: the minima (the bits of fp64 squared distances); WS_IDX: the depths
  if ((rc = c->ws[WS_D2].ensure(nc * sizeof(unsigned long long)))) return rc;
  if ((rc = c->ws[WS_IDX].ensure(nc * sizeof(float)))) return rc;
  unsigned long long* d_min = c->ws[WS_D2].as<unsigned long long>();
  HIPCHK(launch_collide_depth_init(d_min, nc, s));
  if (F) {
    QueryArgs a;
    if ((rc = collide_prepare(c, t.get(), model, P, frames, F, F * P, radius, a))) return rc;
    a.dmin = d_min;
    HIPCHK(launch_collide_depth_axis(a, s));
  }
  HIPCHK(launch_collide_depth_finish(d_min, nc, c->ws[WS_IDX].as<float>(), s));
  HIPCHK(hipMemcpyAsync(dist, c->ws[WS_IDX].p, nc * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return TDTK_OK;
}

}  // extern "C"

// ---- radius clustering (query.hip, "radius clustering"; cluster_lane.h) ---------------------------------------------------
static std::atomic<int> g_cluster_grid_cap{0};

extern "C" {

int tdtk_cluster_grid_cap(int blocks)
{
  return g_cluster_grid_cap.exchange(blocks > 0 ? blocks : 0, std::memory_order_relaxed);
}

int tdtk_cluster_radius(const tdtk_tree* t, double sqRad2, const uint8_t* subset, const double* normals, double min_abs_cos,
                        uint32_t min_size, int32_t* labels, uint64_t* n_clusters, int32_t* first, uint32_t* sizes)
{
  if (!t || !labels || !n_clusters) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (!std::isfinite(sqRad2)) { set_error("sqRad2 must be finite"); return TDTK_EINVAL; }
  if (normals && !(min_abs_cos >= 0.0 && min_abs_cos <= 1.0)) { set_error("min_abs_cos must lie in [0, 1]"); return TDTK_EINVAL; }
  Ctx* c;
  int rc;
  if ((rc = get_ctx(t->device, &c))) return rc;
  hipStream_t s = c->stream;
  const size_t M = t->M, S = t->dev.n_slots;
  // WS_KPOS: parent | ckey | csize, by slot.  WS_D2: cflag | cnum, [M + 1] each.  WS_IDX: labels | first | sizes, [M] each.
  // WS_TMPA: the normals, WS_TMPB: the subset.  Nothing here has the size of a neighbour list
  const size_t tmpb = scan_u32_temp_bytes(M + 1);
  if ((rc = c->ws[WS_KPOS].ensure(3 * S * sizeof(uint32_t)))) return rc;
  if ((rc = c->ws[WS_D2].ensure(2 * (M + 1) * sizeof(uint32_t)))) return rc;
  if ((rc = c->ws[WS_IDX].ensure(3 * M * sizeof(uint32_t)))) return rc;
  if ((rc = c->ws[WS_ARENA].ensure(tmpb + 256))) return rc;
  if (normals && (rc = c->ws[WS_TMPA].ensure(3 * M * sizeof(double)))) return rc;
  if (subset && (rc = c->ws[WS_TMPB].ensure(M))) return rc;
  QueryArgs a{};
  a.nodes = t->dev.nodes; a.pts = t->dev.pts; a.leaf_tab = t->dev.leaf_tab;
  a.root_ref = t->dev.root_ref; a.cb = t->dev.cb; a.cmask = t->dev.cmask;
  a.n = S;
  a.r2 = sqRad2;
  a.parent = c->ws[WS_KPOS].as<uint32_t>(); a.ckey = a.parent + S; a.csize = a.ckey + S;
  a.cflag = c->ws[WS_D2].as<uint32_t>();
  uint32_t* d_num = a.cflag + (M + 1);
  a.cnum = d_num;
  a.labels = c->ws[WS_IDX].as<int32_t>(); a.cfirst = a.labels + M; a.csizes_out = reinterpret_cast<uint32_t*>(a.cfirst + M);
  a.min_size = min_size;
  if (subset) {
    HIPCHK(hipMemcpyAsync(c->ws[WS_TMPB].p, subset, M, hipMemcpyHostToDevice, s));
    a.subset = c->ws[WS_TMPB].as<uint8_t>();
  }
  if (normals) {
    HIPCHK(hipMemcpyAsync(c->ws[WS_TMPA].p, normals, 3 * M * sizeof(double), hipMemcpyHostToDevice, s));
    a.cnormals = c->ws[WS_TMPA].as<double>();
    a.min_cos = min_abs_cos;
  }
  HIPCHK(launch_cluster_init(a, s));
  if (sqRad2 > 0) {      // otherwise no Dist2 is below it: every list is empty, every node a component of its own
    const size_t ovf = query_overflow_entries(S, t->info.max_depth);
    if (ovf) {
      if ((rc = c->ws[WS_OVF_M2].ensure(ovf * sizeof(double)))) return rc;
      if ((rc = c->ws[WS_OVF_REF].ensure(ovf * sizeof(uint32_t)))) return rc;
      a.ovf_m2 = c->ws[WS_OVF_M2].as<double>();
      a.ovf_ref = c->ws[WS_OVF_REF].as<uint32_t>();
    }
    const bool timed = walk_timed();    // tdtk_last_kernel_ms: the link walk
    if (timed) HIPCHK(hipEventRecord(c->e0, s));
    HIPCHK(launch_cluster_link(a, (uint32_t)g_cluster_grid_cap.load(std::memory_order_relaxed), s));
    if (timed) { HIPCHK(hipEventRecord(c->e1, s)); c->ev_pending = true; }
  }
  HIPCHK(hipMemsetAsync(a.cflag, 0, (M + 1) * sizeof(uint32_t), s));
  HIPCHK(launch_cluster_flatten(a, s));
  HIPCHK(launch_scan_u32(a.cflag, d_num, M + 1, c->ws[WS_ARENA].p, tmpb, s));
  HIPCHK(launch_cluster_label(a, s));
  uint32_t n = 0;
  HIPCHK(hipMemcpyAsync(labels, a.labels, M * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&n, d_num + M, sizeof n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *n_clusters = n;
  if (n && (first || sizes)) {
    if (first) HIPCHK(hipMemcpyAsync(first, a.cfirst, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (sizes) HIPCHK(hipMemcpyAsync(sizes, a.csizes_out, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  return TDTK_OK;
}

}  // extern "C"

namespace tdtk {

// The four tree-based normal estimators between their argument checks and their launch, and after it.  Begin: the context,
// the tree over xyz (the points stay in WS_TMPA and are the queries), WS_TMPB for the normals, WS_IDX for `ints` int32 of
// lists and per-point values (0: none), query_prepare, the scanner position.  Finish: the normals, the lists (a.knn_out, L
// int32) and one int32 per point from d_per_point to the host, each where the caller gave an array; then the synchronise
struct NormalsRun {
  Ctx* c;
  std::unique_ptr<tdtk_tree> t;
  QueryArgs a;
  int32_t* ints;
};

static int normals_begin(NormalsRun& r, const double* xyz, size_t n, int bucket, int device, const double rPos[3], size_t ints)
{
  int rc;
  if ((rc = get_ctx(device, &r.c))) return rc;
  Ctx* c = r.c;
  if ((rc = normals_tree(c, xyz, n, bucket, device, r.t))) return rc;
  if ((rc = c->ws[WS_TMPB].ensure(3 * n * sizeof(double)))) return rc;
  if (ints && (rc = c->ws[WS_IDX].ensure(ints * sizeof(int32_t)))) return rc;
  if ((rc = query_prepare(c, r.t.get(), c->ws[WS_TMPA].as<double>(), n, r.a))) return rc;
  r.a.rx = rPos[0]; r.a.ry = rPos[1]; r.a.rz = rPos[2];
  r.a.normals = c->ws[WS_TMPB].as<double>();
  r.ints = ints ? c->ws[WS_IDX].as<int32_t>() : nullptr;
  return TDTK_OK;
}

static int normals_finish(NormalsRun& r, size_t n, double* normals_out, int32_t* lists_out, size_t L, int32_t* per_point_out,
                          const int32_t* d_per_point)
{
  hipStream_t s = r.c->stream;
  HIPCHK(hipMemcpyAsync(normals_out, r.a.normals, 3 * n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (lists_out) HIPCHK(hipMemcpyAsync(lists_out, r.a.knn_out, L * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (per_point_out) HIPCHK(hipMemcpyAsync(per_point_out, d_per_point, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return TDTK_OK;
}

// the argument checks the two adaptive-k estimators share (normals.cc:123-125, 569-571)
int adaptive_check_args(const double* xyz, size_t n, int kmin, int kmax, const double* rPos, const double* normals_out)
{
  if (!rPos) { set_error("rPos is NULL"); return TDTK_EINVAL; }
  if (!xyz || n == 0) { set_error("Could not calculate normals, XYZ data is empty"); return TDTK_EINVAL; }
  if (!normals_out) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (kmin > kmax) { set_error("kmin must not be larger than kmax"); return TDTK_EINVAL; }
  if (kmin < 0) { set_error("kmin must be >= 0"); return TDTK_EINVAL; }
  return TDTK_OK;
}

}  // namespace tdtk

extern "C" {

int tdtk_normals_knn(const double* xyz, size_t n, int k, const double rPos[3], int bucket, int device, double* normals_out,
                     int32_t* knn_out)
{
  if (!rPos) { set_error("rPos is NULL"); return TDTK_EINVAL; }
  if (!xyz || n == 0) { set_error("Could not calculate normals, XYZ data is empty"); return TDTK_EINVAL; }
  if (!normals_out) { set_error("NULL argument"); return TDTK_EINVAL; }
  int rc;
  if ((rc = knn_check_k(k))) return rc;
  const size_t L = knn_out ? n * (size_t)k : 0;
  NormalsRun r;
  if ((rc = normals_begin(r, xyz, n, bucket, device, rPos, L))) return rc;
  r.a.k = k;
  r.a.knn_out = knn_out ? r.ints : nullptr;
  HIPCHK(launch_knn(r.a, true, r.c->stream));
  return normals_finish(r, n, normals_out, knn_out, L, nullptr, nullptr);
}

int tdtk_normals_range(const double* xyz, size_t n, double sqRad2, const double rPos[3], int bucket, int device,
                       double* normals_out)
{
  if (!rPos) { set_error("rPos is NULL"); return TDTK_EINVAL; }
  if (!xyz || n == 0) { set_error("Could not calculate normals, XYZ data is empty"); return TDTK_EINVAL; }
  if (!normals_out) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (!(sqRad2 > 0)) { set_error("sqRad2 must be > 0 (an empty neighbourhood has no mean)"); return TDTK_EINVAL; }
  int rc;
  NormalsRun r;
  if ((rc = normals_begin(r, xyz, n, bucket, device, rPos, 0))) return rc;
  r.a.r2 = sqRad2;
  HIPCHK(launch_range_normals(r.a, r.c->stream));
  return normals_finish(r, n, normals_out, nullptr, 0, nullptr, nullptr);
}

int tdtk_normals_knn_range(const double* xyz, size_t n, int k, double sqRad2, const double rPos[3], int bucket, int device,
                           double* normals_out, int32_t* knn_out, int32_t* counts_out)
{
  if (!rPos) { set_error("rPos is NULL"); return TDTK_EINVAL; }
  if (!xyz || n == 0) { set_error("Could not calculate normals, XYZ data is empty"); return TDTK_EINVAL; }
  if (!normals_out) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (k < 1) { set_error("k must be >= 1"); return TDTK_EINVAL; }
  int rc;
  if ((rc = tree_check_args(n, bucket))) return rc;
  if ((rc = knn_check_k(k))) return rc;
  if (!std::isfinite(sqRad2)) { set_error("sqRad2 must be finite"); return TDTK_EINVAL; }
  if (!(sqRad2 > 0)) { set_error("sqRad2 must be > 0 (an empty neighbourhood has no mean)"); return TDTK_EINVAL; }
  const size_t L = knn_out ? n * (size_t)k : 0;       // WS_IDX: the lists | counts
  NormalsRun r;
  if ((rc = normals_begin(r, xyz, n, bucket, device, rPos, L + n))) return rc;
  r.a.k = k;
  r.a.r2 = sqRad2;
  r.a.knn_out = knn_out ? r.ints : nullptr;
  r.a.nr_out = counts_out ? r.ints + L : nullptr;
  HIPCHK(launch_knn_range(r.a, true, r.c->stream));
  return normals_finish(r, n, normals_out, knn_out, L, counts_out, r.a.nr_out);
}

int tdtk_normals_adaptive_knn(const double* xyz, size_t n, int kmin, int kmax, const double rPos[3], int bucket, int device,
                              double* normals_out, int32_t* k_used, int32_t* knn_out)
{
  int rc;
  if ((rc = adaptive_check_args(xyz, n, kmin, kmax, rPos, normals_out))) return rc;
  if ((rc = tree_check_args(n, bucket))) return rc;
  if (kmax > KNN_MAX_K - 1) {
    set_error("kmax + 1 = " + std::to_string((long long)kmax + 1) + " exceeds the supported list capacity of " + std::to_string(KNN_MAX_K));
    return TDTK_EUNSUP;
  }
  const size_t L = knn_out ? n * (size_t)(kmax + 1) : 0;       // WS_IDX: the lists | k_used
  NormalsRun r;
  if ((rc = normals_begin(r, xyz, n, bucket, device, rPos, L + n))) return rc;
  r.a.kmin = kmin; r.a.kmax = kmax;
  r.a.knn_out = knn_out ? r.ints : nullptr;
  r.a.k_used = k_used ? r.ints + L : nullptr;
  HIPCHK(launch_knn_adaptive(r.a, r.c->stream));
  return normals_finish(r, n, normals_out, knn_out, L, k_used, r.a.k_used);
}

}  // extern "C"
