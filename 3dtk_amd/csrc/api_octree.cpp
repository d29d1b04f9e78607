// The octree entry points: tdtk_octree_create / _create_from_scan / _destroy / _get_info / _leaf_order, tdtk_octree_find_closest
// (and _dev) and tdtk_octree_get_pt_pairs (kernels: octree.hip and, for keys, sort and within-leaf order, reduce.hip; per-lane
// code: oct_lane.h); tdtk_icp_match_octree / _rnd: the octree's pass of an ICP iteration inside api_icp.cpp's loop.
#include "api_internal.h"
#include "octree.h"

using namespace tdtk;

struct tdtk_octree {
  int device = 0;
  size_t n = 0;
  void *d_nodes = nullptr, *d_pts = nullptr;
  OctView view{};
  tdtk_octree_info info{};
  // what the pair-sum kernels, the index scatter and the bin read of a tdtk_tree: the leaf-ordered points, their number,
  // the box and the accumulation point.  It owns nothing.
  tdtk_tree kd;
  tdtk_octree() = default;
  tdtk_octree(const tdtk_octree&) = delete;
  tdtk_octree& operator=(const tdtk_octree&) = delete;
  ~tdtk_octree()
  {
    (void)hipSetDevice(device);
    if (d_nodes) pool_free(d_nodes);
    if (d_pts) pool_free(d_pts);
  }
};

namespace {

// the tree of the n points at WS_TMPA (device, caller order)
int octree_from_device_points(Ctx* c, tdtk_octree* t, size_t n, double voxel_size, int earlystop, double t0)
{
  int rc;
  hipStream_t s = c->stream;
  const size_t sort_tmp = oct_sort_temp_bytes(n), scan_tmp = scan_u32_temp_bytes(n + 1), scan64_tmp = scan_u64_temp_bytes(n + 1);
  const size_t tmpb = std::max(sort_tmp, std::max(scan_tmp, scan64_tmp));
  if ((rc = c->ws[WS_QX].ensure(2 * n * sizeof(uint64_t)))) return rc;           // keys by point | sorted
  if ((rc = c->ws[WS_CELL].ensure(4 * (n + 1) * sizeof(uint32_t)))) return rc;   // flags | ranks of two levels
  if ((rc = c->ws[WS_TMPB].ensure(tmpb + 256))) return rc;
  if ((rc = c->ws[WS_BOX].ensure(bbox_temp_bytes() + 8 * sizeof(double)))) return rc;
  if ((rc = c->ws[WS_QY].ensure(6 * n * sizeof(uint32_t)))) return rc;           // perm | segS segE mid posL posR
  if ((rc = c->ws[WS_QZ].ensure(2 * (n + 1) * sizeof(uint64_t)))) return rc;     // partition flags | their scan
  if ((rc = c->ws[WS_HIST].ensure(32 * sizeof(uint32_t) + n))) return rc;        // counts | leaf depth per sorted position
  double* d_in = c->ws[WS_TMPA].as<double>();
  double* d_box = c->ws[WS_BOX].as<double>();
  uint64_t* keys_a = c->ws[WS_QX].as<uint64_t>();
  uint64_t* keys_b = keys_a + n;
  uint32_t* lv[4];
  for (int k = 0; k < 4; k++) lv[k] = c->ws[WS_CELL].as<uint32_t>() + (size_t)k * (n + 1);
  uint32_t* perm = c->ws[WS_QY].as<uint32_t>();
  uint32_t* work = perm + n;
  uint64_t* f64 = c->ws[WS_QZ].as<uint64_t>();
  uint64_t* P64 = f64 + (n + 1);
  uint32_t* d_counts = c->ws[WS_HIST].as<uint32_t>();
  uint8_t* d_ld = reinterpret_cast<uint8_t*>(d_counts + 32);

  HIPCHK(launch_bbox(d_in, n, d_box + 8, d_box, s, d_box + 6));
  HIPCHK(hipMemcpyAsync(c->h_pin + Ctx::PIN_BOX, d_box, 7 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const double* b = c->h_pin + Ctx::PIN_BOX;
  if (b[6] != 0.0) { set_error("non-finite coordinates"); return TDTK_EINVAL; }
  tdtk_octree_info& I = t->info;
  OctRoot R;                          // the root cube, Boctree.h:248-255
  for (int a = 0; a < 3; a++) R.center[a] = 0.5 * (b[a] + b[3 + a]);
  R.size = std::max(std::max(0.5 * (b[3] - b[0]), 0.5 * (b[4] - b[1])), 0.5 * (b[5] - b[2]));
  R.size += 1.0;
  if (!std::isfinite(R.size)) { set_error("non-finite coordinates"); return TDTK_EINVAL; }
  // init(), Boctree.h:333-356
  I.real_voxelSize = R.size;
  I.max_depth = 1;
  while (I.real_voxelSize > voxel_size && I.max_depth <= OCT_MAX_LEVELS + 1) { I.real_voxelSize = I.real_voxelSize / 2.0; I.max_depth++; }
  // the root's children exist unconditionally; a child is a leaf once its size <= voxelSize (:1168)
  R.depth = I.max_depth > 1 ? I.max_depth - 1 : 1;
  if (R.depth > OCT_MAX_LEVELS) { set_error("voxel size too small for this extent (more than 21 octree levels)"); return TDTK_EUNSUP; }
  I.mult = 1.0 / I.real_voxelSize;
  for (int a = 0; a < 3; a++) { I.center[a] = R.center[a]; I.add[a] = -R.center[a] + R.size; }
  I.size = R.size;
  I.largest_index = (int32_t)((1u << (I.max_depth - 1)) * 2u - 1u);
  I.voxel_size = voxel_size; I.earlystop = earlystop ? 1 : 0; I.levels = R.depth; I.n_points = n;

  HIPCHK(launch_oct_keys_sorted(d_in, n, R, keys_a, keys_b, c->ws[WS_TMPB].p, sort_tmp, s));
  HIPCHK(hipMemsetAsync(d_counts, 0, 32 * sizeof(uint32_t), s));
  HIPCHK(launch_oct_leaf_depth(keys_b, n, R.depth, I.earlystop, d_ld, d_counts, s));
  uint32_t h_counts[32];
  HIPCHK(hipMemcpyAsync(h_counts, d_counts, sizeof h_counts, hipMemcpyDeviceToHost, s));
  HIPCHK(launch_oct_mask_keys(keys_a, keys_b, d_ld, n, R.depth, s));
  HIPCHK(launch_oct_mask_sorted(keys_b, d_ld, n, R.depth, s));
  HIPCHK(launch_oct_leaf_order(keys_a, keys_b, n, R.depth, perm, work, f64, P64, c->ws[WS_TMPB].p, scan64_tmp, s));
  HIPCHK(hipStreamSynchronize(s));
  uint64_t base[OCT_MAX_LEVELS + 2];      // first slot of every depth; the root is slot 0
  base[0] = 0; base[1] = 1;
  for (int L = 1; L <= R.depth; L++) base[L + 1] = base[L] + h_counts[L];
  const uint64_t slots = base[R.depth + 1];
  if (slots >= (1ull << 32)) { set_error("octree too large (32-bit node slots)"); return TDTK_EUNSUP; }
  I.n_leaves = h_counts[31];
  I.n_nodes = slots - I.n_leaves;
  HIPCHK(handle_malloc(&t->d_nodes, (size_t)slots * sizeof(OctNode)));
  HIPCHK(handle_malloc(&t->d_pts, n * sizeof(KdPoint)));
  OctNode* nodes = static_cast<OctNode*>(t->d_nodes);
  HIPCHK(hipMemsetAsync(nodes, 0, (size_t)slots * sizeof(OctNode), s));
  for (int L = 1; L <= R.depth; L++) {
    uint32_t *flags = lv[2 * (L & 1)], *rank = lv[2 * (L & 1) + 1], *pflags = lv[2 * ((L - 1) & 1)], *prank = lv[2 * ((L - 1) & 1) + 1];
    HIPCHK(launch_oct_level_flags(keys_b, d_ld, n, R.depth, L, flags, s));
    HIPCHK(launch_scan_u32(flags, rank, n + 1, c->ws[WS_TMPB].p, scan_tmp, s));
    OctEmit e{};
    e.sorted = keys_b; e.ld = d_ld; e.flags = flags; e.rank = rank; e.pflags = pflags; e.prank = prank;
    e.nodes = nodes; e.base = (uint32_t)base[L]; e.pbase = (uint32_t)base[L - 1]; e.n = (uint32_t)n; e.depth = R.depth; e.L = L;
    HIPCHK(launch_oct_level_emit(e, s));
  }
  HIPCHK(launch_oct_points(d_in, perm, n, static_cast<KdPoint*>(t->d_pts), s));
  HIPCHK(hipStreamSynchronize(s));

  t->n = n;
  OctView& V = t->view;
  V.nodes = nodes; V.pts = static_cast<const KdPoint*>(t->d_pts);
  for (int a = 0; a < 3; a++) V.add[a] = I.add[a];
  V.mult = I.mult; V.largest_index = I.largest_index; V.top_bit = 1u << (I.max_depth - 1);
  t->kd.device = t->device; t->kd.M = n; t->kd.Mp = n;
  t->kd.dev.pts = V.pts; t->kd.dev.n_slots = (uint32_t)n;
  for (int a = 0; a < 3; a++) { t->kd.bbmin[a] = b[a]; t->kd.bbmax[a] = b[3 + a]; t->kd.centre[a] = R.center[a]; }
  I.device_bytes = slots * sizeof(OctNode) + n * sizeof(KdPoint);
  I.build_ms = now_ms() - t0;
  return TDTK_OK;
}

int octree_check_args(size_t n, double voxel_size, tdtk_octree** out)
{
  if (!out) { set_error("out is NULL"); return TDTK_EINVAL; }
  *out = nullptr;
  if (n == 0) { set_error("cannot create an octree with zero points"); return TDTK_EINVAL; }
  if (!(voxel_size > 0)) { set_error("voxel size must be > 0"); return TDTK_EINVAL; }
  if (n >= (1ull << 31)) { set_error("scan too large"); return TDTK_EINVAL; }
  return TDTK_OK;
}

// the range rule of the header: sqrt(maxdist2) * mult + 1 on the host, the queries' voxel coordinates on the device
int octree_radius_check(const tdtk_octree* t, double maxd2)
{
  if (!(std::fabs(std::sqrt(maxd2) * t->view.mult + 1) < OCT_INT_LIMIT)) {       // oct_in_range; a NaN: refused
    set_error("sqrt(maxdist2) * mult + 1 does not fit +-2^30: the reference's int conversion is undefined");
    return TDTK_EUNSUP;
  }
  return TDTK_OK;
}

// the search over the sorted queries a.x / a.y / a.z (inv: moved by it first, into WS_DX / WS_DY / WS_DZ): the prepare pass
// with its range check (one look at the device), then the walk
int octree_run_search(Ctx* c, const tdtk_octree* t, OctSearchArgs& a, const double* inv, hipStream_t s)
{
  int rc;
  if ((rc = c->ws[WS_CNT].ensure(64))) return rc;
  OctPrepArgs p{};
  p.x = a.x; p.y = a.y; p.z = a.z; p.n = a.n;
  if (inv) {
    int ids[] = {WS_DX, WS_DY, WS_DZ};
    for (int id : ids)
      if ((rc = c->ws[id].ensure(a.n * sizeof(double)))) return rc;
    p.ox = c->ws[WS_DX].as<double>(); p.oy = c->ws[WS_DY].as<double>(); p.oz = c->ws[WS_DZ].as<double>();
    std::memcpy(p.inv.m, inv, sizeof p.inv.m);
    p.has_inv = 1;
    a.x = p.ox; a.y = p.oy; a.z = p.oz;
  }
  for (int k = 0; k < 3; k++) p.add[k] = t->view.add[k];
  p.mult = t->view.mult;
  p.bad = c->ws[WS_CNT].as<uint32_t>();
  a.T = t->view; a.levels = t->info.levels;
  HIPCHK(hipMemsetAsync(p.bad, 0, sizeof(uint32_t), s));
  HIPCHK(launch_oct_prepare(p, s));
  uint32_t bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, p.bad, sizeof bad, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (bad) {
    set_error("a query's voxel coordinate (q + add) * mult does not fit +-2^30: the reference's int conversion is undefined");
    return TDTK_EUNSUP;
  }
  HIPCHK(launch_oct_search(a, s));
  return TDTK_OK;
}

// Scan::getPtPairs over a resident scan, FindClosest being the octree's: search, then scan_pass's sums over (query, hit slot)
int octree_scan_pairs(const tdtk_octree* t, const double A[16], tdtk_scan* data, int pmode, double maxd2, uint32_t want,
                      const double* lum_D, int32_t* idx_out, tdtk_pair_sums* sums)
{
  if (t->device != data->device) { set_error("tree and scan live on different devices"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(t->device, &c);
  if (rc) return rc;
  std::memset(sums, 0, sizeof *sums);
  sums->n_queries = data->N;
  if (data->N == 0) return TDTK_OK;
  if ((rc = c->ws[WS_KPOS].ensure(data->N * sizeof(int)))) return rc;
  if ((rc = scan_settle(c, data))) return rc;
  OctSearchArgs a{};
  a.x = data->x; a.y = data->y; a.z = data->z; a.n = data->N;
  double inv[16];
  m4inv(A, inv);              // searchTree.cc:110
  a.maxd2 = maxd2;
  a.kpos = c->ws[WS_KPOS].as<int>();
  if ((rc = octree_run_search(c, t, a, inv, c->stream))) return rc;
  c->cert_live = false;       // WS_KPOS no longer holds a k-d pass's hits
  double acc[ACC_TOTAL], shift[3];
  if ((rc = scan_pass(c, &t->kd, A, data, pmode, maxd2, want, lum_D, nullptr, false, acc, shift))) return rc;
  finish_sums(acc, shift, data->N, want, sums);
  if (lum_D) sums->lum_sumd2 = acc[ACC_LSS];
  if (idx_out) rc = scan_idx_to_host(c, &t->kd, data, idx_out);
  return rc;
}

// One iteration of tdtk_icp_match_octree: the loop-form prepare pass (moves the scan by `pending`, the tree-frame coordinates
// into WS_DX / WS_DY / WS_DZ, the range word), the walk, the range word on its way to pinned memory, then scan_pass's sums over
// (query, hit slot) -- whose wait is the only one: the host looks at the range word once the sums are there.
int octree_loop_pass(Ctx* c, const tdtk_octree* t, const double A[16], tdtk_scan* data, int pmode, double maxd2, unsigned want,
                     const double* pending, const unsigned char* skip, double* acc, double shift[3])
{
  int rc;
  hipStream_t s = c->stream;
  const size_t N = data->N;
  if ((rc = c->ws[WS_KPOS].ensure(N * sizeof(int))) || (rc = c->ws[WS_CNT].ensure(64))) return rc;
  int ids[] = {WS_DX, WS_DY, WS_DZ};
  for (int id : ids)
    if ((rc = c->ws[id].ensure(N * sizeof(double)))) return rc;
  if ((rc = scan_settle(c, data))) return rc;
  OctLoopPrepArgs p{};
  p.x = data->x; p.y = data->y; p.z = data->z;
  p.nx = data->nx; p.ny = data->ny; p.nz = data->nz;
  p.ox = c->ws[WS_DX].as<double>(); p.oy = c->ws[WS_DY].as<double>(); p.oz = c->ws[WS_DZ].as<double>();
  p.n = N;
  p.has_pending = pending ? 1 : 0;
  if (pending) std::memcpy(p.pending.m, pending, sizeof p.pending.m);
  m4inv(A, p.inv.m);          // searchTree.cc:110
  for (int k = 0; k < 3; k++) p.add[k] = t->view.add[k];
  p.mult = t->view.mult;
  p.bad = c->ws[WS_CNT].as<uint32_t>();
  OctLoopSearchArgs a{};
  a.T = t->view; a.levels = t->info.levels;
  a.x = p.ox; a.y = p.oy; a.z = p.oz; a.n = N;
  a.maxd2 = maxd2;
  a.kpos = c->ws[WS_KPOS].as<int>();
  a.skip = skip;
  a.bad = p.bad;
  uint32_t* h_bad = reinterpret_cast<uint32_t*>(c->h_pin + Ctx::PIN_OCT_RANGE);
  HIPCHK(hipMemsetAsync(p.bad, 0, sizeof(uint32_t), s));
  HIPCHK(launch_oct_loop_prepare(p, s));
  const bool timed = kernel_timing();
  if (timed) HIPCHK(hipEventRecord(c->e0, s));
  HIPCHK(launch_oct_loop_search(a, s));
  if (timed) { HIPCHK(hipEventRecord(c->e1, s)); c->ev_pending = true; }
  HIPCHK(hipMemcpyAsync(h_bad, p.bad, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  c->cert_live = false;       // WS_KPOS no longer holds a k-d pass's hits
  if ((rc = scan_pass(c, &t->kd, A, data, pmode, maxd2, want, nullptr, nullptr, false, acc, shift))) return rc;
  if (*reinterpret_cast<volatile uint32_t*>(h_bad)) {
    set_error("a query's voxel coordinate (q + add) * mult does not fit +-2^30: the reference's int conversion is undefined");
    return TDTK_EUNSUP;
  }
  return TDTK_OK;
}

int octree_icp_match(const tdtk_octree* model, const double model_dalignxf[16], tdtk_scan* data, double data_transMat[16],
                     double data_dalignxf[16], const tdtk_icp_params* prm, int rnd, tdtk_icp_result* res, double* trace, int trace_cap)
{
  if (!model) { set_error("NULL argument"); return TDTK_EINVAL; }
  IcpTreePass other;
  other.check = [&](int pmode, double maxd2) {
    if (pmode == TDTK_CLOSEST_POINT_ALONG_NORMAL_SIMPLE) {
      set_error("BOctTree has no FindClosestAlongDir of its own (it inherits SearchTree's): pairing mode 1 is not served by the octree");
      return (int)TDTK_EUNSUP;
    }
    if (pmode != TDTK_CLOSEST_POINT && pmode != TDTK_CLOSEST_PLANE_SIMPLE) { set_error("bad pairing mode"); return (int)TDTK_EINVAL; }
    if (model->device != data->device) { set_error("tree and scan live on different devices"); return (int)TDTK_EINVAL; }
    return octree_radius_check(model, maxd2);
  };
  other.pass = [&](const double* pending, const unsigned char* skip, unsigned want, double* acc, double* shift) {
    Ctx* c;
    int rc = get_ctx(model->device, &c);
    if (rc) return rc;
    return octree_loop_pass(c, model, model_dalignxf, data, prm->pairing_mode, prm->max_dist_match2, want, pending, skip, acc, shift);
  };
  return icp_match_loop(&model->kd, &other, model_dalignxf, data, data_transMat, data_dalignxf, prm, rnd, res, trace, trace_cap);
}

}  // namespace

extern "C" {

int tdtk_icp_match_octree(const tdtk_octree* model, const double model_dalignxf[16], tdtk_scan* data, double data_transMat[16],
                          double data_dalignxf[16], const tdtk_icp_params* prm, tdtk_icp_result* res, double* trace, int trace_cap)
{
  return octree_icp_match(model, model_dalignxf, data, data_transMat, data_dalignxf, prm, 1, res, trace, trace_cap);
}
int tdtk_icp_match_octree_rnd(const tdtk_octree* model, const double model_dalignxf[16], tdtk_scan* data, double data_transMat[16],
                              double data_dalignxf[16], const tdtk_icp_params* prm, int rnd, tdtk_icp_result* res, double* trace,
                              int trace_cap)
{
  return octree_icp_match(model, model_dalignxf, data, data_transMat, data_dalignxf, prm, rnd, res, trace, trace_cap);
}

int tdtk_octree_create(const double* xyz, size_t n, double voxel_size, int earlystop, int device, tdtk_octree** out)
{
  int rc;
  if ((rc = octree_check_args(n, voxel_size, out))) return rc;
  if (!xyz) { set_error("NULL points"); return TDTK_EINVAL; }
  Ctx* c;
  if ((rc = get_ctx(device, &c))) return rc;
  const double t0 = now_ms();
  std::unique_ptr<tdtk_octree> t(new tdtk_octree);
  t->device = device;
  if ((rc = c->ws[WS_TMPA].ensure(3 * n * sizeof(double)))) return rc;
  HIPCHK(hipMemcpyAsync(c->ws[WS_TMPA].p, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = octree_from_device_points(c, t.get(), n, voxel_size, earlystop, t0))) return rc;
  *out = t.release();
  return TDTK_OK;
}

int tdtk_octree_create_from_scan(const tdtk_scan* scan, double voxel_size, int earlystop, tdtk_octree** out)
{
  int rc;
  if ((rc = octree_check_args(scan ? scan->N : 0, voxel_size, out))) return rc;
  Ctx* c;
  if ((rc = get_ctx(scan->device, &c))) return rc;
  const double t0 = now_ms();
  const size_t n = scan->N;
  std::unique_ptr<tdtk_octree> t(new tdtk_octree);
  t->device = scan->device;
  if ((rc = c->ws[WS_TMPA].ensure(3 * n * sizeof(double)))) return rc;
  const bool saved = scan->ox != nullptr;   // moved since tdtk_scan_mark_original: the saved points are the original
  if (!saved && (rc = scan_settle(c, scan))) return rc;
  HIPCHK(launch_unsort_aos(saved ? scan->ox : scan->x, saved ? scan->oy : scan->y, saved ? scan->oz : scan->z,
                           scan->d_order, n, c->ws[WS_TMPA].as<double>(), c->stream));
  if ((rc = octree_from_device_points(c, t.get(), n, voxel_size, earlystop, t0))) return rc;
  *out = t.release();
  return TDTK_OK;
}

void tdtk_octree_destroy(tdtk_octree* t) { delete t; }

int tdtk_octree_get_info(const tdtk_octree* t, tdtk_octree_info* info)
{
  if (!t || !info) { set_error("NULL argument"); return TDTK_EINVAL; }
  *info = t->info;
  return TDTK_OK;
}

int tdtk_octree_leaf_order(const tdtk_octree* t, int32_t* order)
{
  if (!t || !order) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(t->device, &c);
  if (rc) return rc;
  std::vector<KdPoint> pts(t->n);
  HIPCHK(hipMemcpyAsync(pts.data(), t->d_pts, t->n * sizeof(KdPoint), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < t->n; i++) order[i] = pts[i].orig;
  return TDTK_OK;
}

int tdtk_octree_node_table(const tdtk_octree* t, uint32_t* table, size_t cap, uint64_t* slots)
{
  if (!t || !slots) { set_error("NULL argument"); return TDTK_EINVAL; }
  *slots = t->info.n_nodes + t->info.n_leaves;
  if (!table) return TDTK_OK;
  if (cap < *slots) { set_error("cap " + std::to_string(cap) + " < slots " + std::to_string(*slots)); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(t->device, &c);
  if (rc) return rc;
  static_assert(sizeof(OctNode) == 4 * sizeof(uint32_t), "a slot is four words");
  HIPCHK(hipMemcpyAsync(table, t->d_nodes, (size_t)*slots * sizeof(OctNode), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TDTK_OK;
}

int tdtk_octree_find_closest_dev(const tdtk_octree* t, const double* d_q, size_t K, double maxdist2, int32_t* d_idx, double* d_d2,
                                 void* stream)
{
  if (!t || ((!d_q || !d_idx) && K)) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(t->device, &c);
  if (rc) return rc;
  if ((rc = octree_radius_check(t, maxdist2))) return rc;
  if (K == 0) return TDTK_OK;
  if (K >= (1ull << 31)) { set_error("too many queries for one call"); return TDTK_EUNSUP; }
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  int ids[] = {WS_QX, WS_QY, WS_QZ, WS_D2};
  for (int id : ids)
    if ((rc = c->ws[id].ensure(K * sizeof(double)))) return rc;
  if ((rc = c->ws[WS_KPOS].ensure(K * sizeof(int)))) return rc;
  if ((rc = c->ws[WS_ORDER].ensure(K * sizeof(int32_t)))) return rc;
  if ((rc = c->ws[WS_CELL].ensure(K * sizeof(uint32_t)))) return rc;
  if ((rc = c->ws[WS_HIST].ensure(32768 * sizeof(uint32_t)))) return rc;
  BinArgs b{};               // the batch in spatial order: 32 cells per axis over the points' box
  b.q = d_q; b.n = K;
  for (int ax = 0; ax < 3; ax++) {
    b.lo[ax] = t->kd.bbmin[ax];
    const double ext = t->kd.bbmax[ax] - t->kd.bbmin[ax];
    b.scale[ax] = (ext > 0) ? 32.0 / ext : 0.0;
  }
  b.hist = c->ws[WS_HIST].as<uint32_t>();
  b.cell = c->ws[WS_CELL].as<uint32_t>();
  b.sx = c->ws[WS_QX].as<double>(); b.sy = c->ws[WS_QY].as<double>(); b.sz = c->ws[WS_QZ].as<double>();
  b.order = c->ws[WS_ORDER].as<int32_t>();
  HIPCHK(launch_bin(b, s));
  OctSearchArgs a{};
  a.x = b.sx; a.y = b.sy; a.z = b.sz; a.n = K;
  a.maxd2 = maxdist2;
  a.kpos = c->ws[WS_KPOS].as<int>();
  a.d2 = c->ws[WS_D2].as<double>();
  if ((rc = octree_run_search(c, t, a, nullptr, s))) return rc;
  c->cert_live = false;
  HIPCHK(launch_scatter_idx(a.kpos, a.d2, b.order, t->view.pts, K, d_idx, d_d2, s));
  if (!stream) HIPCHK(hipStreamSynchronize(s));
  else {
    // the kernels queued on the caller's stream use this thread's workspaces: whatever this thread's own stream does next
    // waits for them (as tdtk_find_closest_dev)
    HIPCHK(hipEventRecord(c->e_user, s));
    HIPCHK(hipStreamWaitEvent(c->stream, c->e_user, 0));
  }
  return TDTK_OK;
}

int tdtk_octree_find_closest(const tdtk_octree* t, const double* q, size_t K, double maxdist2, int32_t* idx, double* d2)
{
  if (!t || ((!q || !idx) && K)) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(t->device, &c);
  if (rc) return rc;
  if ((rc = octree_radius_check(t, maxdist2))) return rc;
  if (K == 0) return TDTK_OK;
  if ((rc = c->ws[WS_TMPA].ensure(3 * K * sizeof(double)))) return rc;
  if ((rc = c->ws[WS_IDX].ensure(K * sizeof(int32_t)))) return rc;
  if ((rc = c->ws[WS_TMPB].ensure(K * sizeof(double)))) return rc;
  HIPCHK(hipMemcpyAsync(c->ws[WS_TMPA].p, q, 3 * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
  rc = tdtk_octree_find_closest_dev(t, c->ws[WS_TMPA].as<double>(), K, maxdist2, c->ws[WS_IDX].as<int32_t>(),
                                    c->ws[WS_TMPB].as<double>(), c->stream);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(idx, c->ws[WS_IDX].p, K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (d2) HIPCHK(hipMemcpyAsync(d2, c->ws[WS_TMPB].p, K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TDTK_OK;
}

int tdtk_octree_get_pt_pairs(const tdtk_octree* t, const double A[16], const double* xyz_r, const double* normal_r, size_t start,
                             size_t end, int rnd, int pmode, double maxd2, uint32_t want, const double* lum_D, int32_t* idx_out,
                             double* p1_out, double* p2_out, double* pn_out, tdtk_pair_sums* sums)
{
  if (!t) { set_error("bad argument"); return TDTK_EINVAL; }
  if (pmode == TDTK_CLOSEST_POINT_ALONG_NORMAL_SIMPLE) {
    set_error("BOctTree has no FindClosestAlongDir of its own (it inherits SearchTree's): pairing mode 1 is not served by the octree");
    return TDTK_EUNSUP;
  }
  if (pmode != TDTK_CLOSEST_POINT && pmode != TDTK_CLOSEST_PLANE_SIMPLE) { set_error("bad pairing mode"); return TDTK_EINVAL; }
  int rc;
  if ((rc = octree_radius_check(t, maxd2))) return rc;
  const PairsPass pass = [&](tdtk_scan* sc, int32_t* idx, tdtk_pair_sums* o) {
    if ((pmode != 0 || (want & TDTK_WANT_NAPX)) && sc->N && !sc->nx) { set_error("this pairing mode / minimizer needs normals"); return (int)TDTK_EINVAL; }
    return octree_scan_pairs(t, A, sc, pmode, maxd2, want, lum_D, idx, o);
  };
  return get_pt_pairs_over(&t->kd, pass, A, xyz_r, normal_r, start, end, rnd, pmode, maxd2, want, idx_out, p1_out, p2_out, pn_out, sums);
}

}  // extern "C"
