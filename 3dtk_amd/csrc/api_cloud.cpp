// Raw clouds and resident scans before they are matched: octree reduction (reduce.hip) and point normals from the ANN tree
// (ann.hip).
#include "api_internal.h"

using namespace tdtk;

extern "C" {

// ---- octree reduction ("-r <voxelSize>", centre mode) -----------------------------------
// Scan::calcReducedPoints (scan.cc:577-603) with reduction_nrpts == 0: BOctTree(xyz, n, voxelSize)
// then GetOctTreeCenter.  See reduce.hip.
int tdtk_reduce_octree(const double* xyz, size_t n, double voxel_size, int device, double* out_xyz, size_t* n_out)
{
  if (!n_out) { set_error("n_out is NULL"); return TDTK_EINVAL; }
  *n_out = 0;
  if (n == 0) return TDTK_OK;   // an empty root has no occupied child (Boctree.h:1268-1300)
  if (!xyz || !out_xyz) { set_error("NULL points"); return TDTK_EINVAL; }
  if (!(voxel_size > 0)) { set_error("voxel size must be > 0"); return TDTK_EINVAL; }
  if (n >= (1ull << 32) - 1) { set_error("scan too large"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(device, &c);
  if (rc) return rc;
  hipStream_t s = c->stream;
  const size_t sort_tmp = oct_sort_temp_bytes(n), scan_tmp = scan_u32_temp_bytes(n + 1);
  const size_t tmpb = sort_tmp > scan_tmp ? sort_tmp : scan_tmp;
  if ((rc = c->ws[WS_TMPA].ensure(6 * n * sizeof(double)))) return rc;          // points in | centres out
  if ((rc = c->ws[WS_QX].ensure(2 * n * sizeof(uint64_t)))) return rc;          // keys a|b
  if ((rc = c->ws[WS_CELL].ensure(2 * (n + 1) * sizeof(uint32_t)))) return rc;  // flags | slots
  if ((rc = c->ws[WS_TMPB].ensure(tmpb + 256))) return rc;
  if ((rc = c->ws[WS_BOX].ensure(bbox_temp_bytes() + 8 * sizeof(double)))) return rc;
  double* d_in = c->ws[WS_TMPA].as<double>();
  double* d_out = d_in + 3 * n;
  double* d_box = c->ws[WS_BOX].as<double>();
  uint64_t* keys_a = c->ws[WS_QX].as<uint64_t>();
  uint64_t* keys_b = keys_a + n;
  uint32_t* flags = c->ws[WS_CELL].as<uint32_t>();
  uint32_t* slot = flags + (n + 1);
  HIPCHK(hipMemcpyAsync(d_in, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(launch_bbox(d_in, n, d_box + 8, d_box, s));
  HIPCHK(hipMemcpyAsync(c->h_pin, d_box, 6 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const double* b = c->h_pin;
  // root cube, Boctree.h:248-255
  OctRoot R;
  for (int a = 0; a < 3; a++) R.center[a] = 0.5 * (b[a] + b[3 + a]);
  R.size = std::max(std::max(0.5 * (b[3] - b[0]), 0.5 * (b[4] - b[1])), 0.5 * (b[5] - b[2]));
  R.size += 1.0;
  if (!std::isfinite(R.size)) { set_error("non-finite coordinates"); return TDTK_EINVAL; }
  // the root's children exist unconditionally (:257-268); a child is a leaf once its size <= voxelSize (:1166)
  R.depth = 1;
  for (double sz = R.size / 2.0; sz > voxel_size; sz /= 2.0) R.depth++;
  if (3 * R.depth > 63) { set_error("voxel size too small for this extent (more than 21 octree levels)"); return TDTK_EINVAL; }
  HIPCHK(launch_oct_keys_sorted(d_in, n, R, keys_a, keys_b, c->ws[WS_TMPB].p, sort_tmp, s));
  HIPCHK(launch_oct_heads(keys_b, n, flags, s));
  HIPCHK(launch_scan_u32(flags, slot, n + 1, c->ws[WS_TMPB].p, scan_tmp, s));
  HIPCHK(launch_oct_centres(keys_b, flags, slot, n, R, d_out, s));
  uint32_t cells = 0;
  HIPCHK(hipMemcpyAsync(&cells, slot + n, sizeof cells, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipMemcpyAsync(out_xyz, d_out, 3 * (size_t)cells * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *n_out = cells;
  return TDTK_OK;
}

// Octree reduction with `-O <nrpts>` (Scan::calcReducedPoints, scan.cc:586-596): nrpts == 0 the leaf centres (above),
// nrpts == 1 one random point per occupied leaf (GetOctTreeRandom, Boctree.h:985-1018), nrpts > 1 up to nrpts random points
// per leaf (Boctree.h:1020-1062 with rm_scatter == false).  The leaves, their depth-first order and the order of the
// points inside a leaf are computed on the device (reduce.hip); the draws are std::rand() on the host, leaf by leaf in
// that order, as the reference makes them -- like `rnd`, reproducible against a serial build of the reference only
// (SURVEY N-d).  Not offered: nrpts == -1 (GetOctTreeAvg adds into memory it never initialises, Boctree.h:961-964) and
// rm_scatter (its loop forgets to advance the child pointer for a leaf it skips, Boctree.h:1032-1040).
int tdtk_reduce_octree_nrpts(const double* xyz, size_t n, double voxel_size, int nrpts, int rm_scatter, int device, double* out_xyz,
                             size_t* n_out)
{
  if (nrpts == 0 && !rm_scatter) return tdtk_reduce_octree(xyz, n, voxel_size, device, out_xyz, n_out);
  if (!n_out) { set_error("n_out is NULL"); return TDTK_EINVAL; }
  *n_out = 0;
  if (nrpts < 0) { set_error("reduction_nrpts == -1 (GetOctTreeAvg) reads uninitialised memory in the reference: not reproducible"); return TDTK_EUNSUP; }
  if (rm_scatter) { set_error("rm_scatter walks a stale child pointer in the reference (Boctree.h:1032-1040): not reproducible"); return TDTK_EUNSUP; }
  if (n == 0) return TDTK_OK;
  if (!xyz || !out_xyz) { set_error("NULL points"); return TDTK_EINVAL; }
  if (!(voxel_size > 0)) { set_error("voxel size must be > 0"); return TDTK_EINVAL; }
  if (n >= (1ull << 31)) { set_error("scan too large"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(device, &c);
  if (rc) return rc;
  hipStream_t s = c->stream;
  const size_t sort_tmp = oct_sort_temp_bytes(n), scan_tmp = scan_u32_temp_bytes(n + 1), scan64_tmp = scan_u64_temp_bytes(n + 1);
  const size_t tmpb = std::max(sort_tmp, std::max(scan_tmp, scan64_tmp));
  if ((rc = c->ws[WS_TMPA].ensure(6 * n * sizeof(double)))) return rc;           // points in | points out
  if ((rc = c->ws[WS_QX].ensure(2 * n * sizeof(uint64_t)))) return rc;           // keys by point | sorted
  if ((rc = c->ws[WS_CELL].ensure(3 * (n + 1) * sizeof(uint32_t)))) return rc;   // leaf flags | slots | starts
  if ((rc = c->ws[WS_TMPB].ensure(tmpb + 256))) return rc;
  if ((rc = c->ws[WS_BOX].ensure(bbox_temp_bytes() + 8 * sizeof(double)))) return rc;
  if ((rc = c->ws[WS_QY].ensure(7 * n * sizeof(uint32_t)))) return rc;           // perm | segS segE mid posL posR | sel
  if ((rc = c->ws[WS_QZ].ensure(2 * (n + 1) * sizeof(uint64_t)))) return rc;     // flags | their scan
  double* d_in = c->ws[WS_TMPA].as<double>();
  double* d_out = d_in + 3 * n;
  double* d_box = c->ws[WS_BOX].as<double>();
  uint64_t* keys_a = c->ws[WS_QX].as<uint64_t>();
  uint64_t* keys_b = keys_a + n;
  uint32_t* flags = c->ws[WS_CELL].as<uint32_t>();
  uint32_t* slot = flags + (n + 1);
  uint32_t* starts = slot + (n + 1);
  uint32_t* perm = c->ws[WS_QY].as<uint32_t>();
  uint32_t* work = perm + n;
  uint32_t* d_sel = perm + 6 * n;
  uint64_t* f64 = c->ws[WS_QZ].as<uint64_t>();
  uint64_t* P64 = f64 + (n + 1);
  HIPCHK(hipMemcpyAsync(d_in, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(launch_bbox(d_in, n, d_box + 8, d_box, s));
  HIPCHK(hipMemcpyAsync(c->h_pin, d_box, 6 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const double* b = c->h_pin;
  OctRoot R;                          // root cube, Boctree.h:248-255
  for (int a = 0; a < 3; a++) R.center[a] = 0.5 * (b[a] + b[3 + a]);
  R.size = std::max(std::max(0.5 * (b[3] - b[0]), 0.5 * (b[4] - b[1])), 0.5 * (b[5] - b[2]));
  R.size += 1.0;
  if (!std::isfinite(R.size)) { set_error("non-finite coordinates"); return TDTK_EINVAL; }
  R.depth = 1;
  for (double sz = R.size / 2.0; sz > voxel_size; sz /= 2.0) R.depth++;
  if (3 * R.depth > 63) { set_error("voxel size too small for this extent (more than 21 octree levels)"); return TDTK_EINVAL; }
  HIPCHK(launch_oct_keys_sorted(d_in, n, R, keys_a, keys_b, c->ws[WS_TMPB].p, sort_tmp, s));
  HIPCHK(launch_oct_heads(keys_b, n, flags, s));
  HIPCHK(launch_scan_u32(flags, slot, n + 1, c->ws[WS_TMPB].p, scan_tmp, s));
  HIPCHK(launch_oct_leaf_starts(flags, slot, n, starts, s));
  HIPCHK(launch_oct_leaf_order(keys_a, keys_b, n, R.depth, perm, work, f64, P64, c->ws[WS_TMPB].p, scan64_tmp, s));
  uint32_t cells = 0;
  HIPCHK(hipMemcpyAsync(&cells, slot + n, sizeof cells, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::vector<uint32_t> st((size_t)cells + 1);
  HIPCHK(hipMemcpy(st.data(), starts, st.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  // the draws, leaf by leaf in depth-first order (globals.icc:607-610: rand(rnd) = (int)(rnd * std::rand() / (RAND_MAX + 1.0)))
  auto draw = [](int rnd) { return (int)((double)rnd * (double)std::rand() / (RAND_MAX + 1.0)); };
  std::vector<uint32_t> sel;
  sel.reserve(nrpts == 1 ? cells : n);
  std::vector<int> pick;
  for (uint32_t l = 0; l < cells; l++) {
    const uint32_t start = st[l], len = st[l + 1] - st[l];
    if (nrpts == 1) { sel.push_back(start + (uint32_t)draw((int)len)); continue; }
    if ((uint32_t)nrpts >= len) { for (uint32_t j = 0; j < len; j++) sel.push_back(start + j); continue; }
    pick.clear();
    while ((int)pick.size() < nrpts) {           // std::set<int>::insert of rand(length - 1)
      const int t = draw((int)len - 1);
      if (std::find(pick.begin(), pick.end(), t) == pick.end()) pick.push_back(t);
    }
    std::sort(pick.begin(), pick.end());
    for (int t : pick) sel.push_back(start + (uint32_t)t);
  }
  const size_t m = sel.size();
  if (m > n) { set_error("internal: more points kept than given"); return TDTK_EDEVICE; }
  if (m) {
    HIPCHK(hipMemcpyAsync(d_sel, sel.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIPCHK(launch_oct_gather(d_in, perm, d_sel, m, d_out, s));
    HIPCHK(hipMemcpyAsync(out_xyz, d_out, 3 * m * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  *n_out = m;
  return TDTK_OK;
}

// ---- normals (Scan::calcNormals -> calculateNormalsApxKNN, scan.cc:398-427, normals.cc:35-111) ----------------
// d_xyz: [n][3] in the caller's order (the ANN tree starts from the identity permutation, kd_tree.cpp:259-262);
// d_normals [n][3] and d_knn (nullable, [n][k]) come back in the caller's order.
// the build half: the ANN tree of d_xyz in WS_QX (nodes) / WS_QY (points) / WS_BOX (the root cell), and the search's spill
// area in WS_OVF_REF / WS_OVF_M2 sized for ann_search_threads(n)
struct AnnTreeDev {
  AnnNode* nodes;
  KdPoint* pts;
  double* d_bb;
  uint32_t root_ref, max_depth;
};
static int ann_tree_on_device(Ctx* c, const double* d_xyz, size_t n, AnnTreeDev& t)
{
  int rc;
  hipStream_t s = c->stream;
  if ((rc = c->ws[WS_ARENA].ensure(ann_build_arena_bytes(n)))) return rc;
  if ((rc = c->ws[WS_QX].ensure((n ? n : 1) * sizeof(AnnNode)))) return rc;
  if ((rc = c->ws[WS_QY].ensure(n * sizeof(KdPoint)))) return rc;
  if ((rc = c->ws[WS_BOX].ensure(bbox_temp_bytes() + 8 * sizeof(double)))) return rc;
  t.nodes = c->ws[WS_QX].as<AnnNode>();
  t.pts = c->ws[WS_QY].as<KdPoint>();
  t.d_bb = c->ws[WS_BOX].as<double>();
  AnnBuildResult r = ann_build_tree(d_xyz, n, c->ws[WS_ARENA].p, t.nodes, t.pts, t.d_bb, s);
  if (r.err != hipSuccess) {
    if (r.degenerate) { set_error("non-finite coordinates"); return TDTK_EINVAL; }
    set_error(std::string("ann_build_tree: ") + hipGetErrorString(r.err));
    return TDTK_EDEVICE;
  }
  t.root_ref = r.root_ref; t.max_depth = r.max_depth;
  const size_t spill = ann_spill_entries(n, r.max_depth);
  if ((rc = c->ws[WS_OVF_REF].ensure((spill + 1) * sizeof(uint32_t)))) return rc;
  if ((rc = c->ws[WS_OVF_M2].ensure((spill + 1) * sizeof(double)))) return rc;
  return TDTK_OK;
}

static int normals_on_device(Ctx* c, const double* d_xyz, size_t n, int k, const double rPos[3], double eps,
                             double* d_normals, int32_t* d_knn)
{
  int rc;
  hipStream_t s = c->stream;
  AnnTreeDev t;
  if ((rc = ann_tree_on_device(c, d_xyz, n, t))) return rc;
  unsigned long long* d_cnt = nullptr;
  if (c->counting) { d_cnt = c->d_counters.as<unsigned long long>() + 4; c->counted_ann_queries += n; }
  HIPCHK(hipEventRecord(c->e4, s));
  HIPCHK(launch_ann_normals(t.nodes, t.root_ref, t.pts, n, k, eps, t.d_bb, rPos, c->ws[WS_OVF_REF].as<uint32_t>(),
                            c->ws[WS_OVF_M2].as<double>(), t.max_depth, d_normals, d_knn, d_cnt, s));
  HIPCHK(hipEventRecord(c->e5, s));
  c->ev4_pending = true;
  return TDTK_OK;
}

static int normals_check_args(size_t n, int k, const double* rPos, double eps)
{
  if (!rPos) { set_error("rPos is NULL"); return TDTK_EINVAL; }
  if (n == 0) { set_error("Could not calculate normals, XYZ data is empty"); return TDTK_EINVAL; }   // scan.cc:408-409
  if (k < 1 || k > 32) { set_error("k must be in 1..32"); return TDTK_EINVAL; }
  if ((size_t)k > n) { set_error("Requesting more near neighbors than data points"); return TDTK_EINVAL; }   // kd_search.cpp:103-105
  if (!(eps >= 0) || !std::isfinite(eps)) { set_error("eps must be >= 0"); return TDTK_EINVAL; }
  if (n >= (1ull << 29)) { set_error("scan too large (29-bit point positions)"); return TDTK_EINVAL; }
  return TDTK_OK;
}

int tdtk_normals_apx_knn(const double* xyz, size_t n, int k, const double rPos[3], double eps, int device,
                         double* normals_out, int32_t* knn_out)
{
  int rc;
  if ((rc = normals_check_args(n, k, rPos, eps))) return rc;
  if (!xyz || !normals_out) { set_error("NULL points"); return TDTK_EINVAL; }
  Ctx* c;
  if ((rc = get_ctx(device, &c))) return rc;
  hipStream_t s = c->stream;
  if ((rc = c->ws[WS_TMPA].ensure(6 * n * sizeof(double)))) return rc;   // points in | normals out
  if (knn_out && (rc = c->ws[WS_IDX].ensure(n * (size_t)k * sizeof(int32_t)))) return rc;
  double* d_in = c->ws[WS_TMPA].as<double>();
  double* d_nrm = d_in + 3 * n;
  int32_t* d_knn = knn_out ? c->ws[WS_IDX].as<int32_t>() : nullptr;
  HIPCHK(hipMemcpyAsync(d_in, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, s));
  if ((rc = normals_on_device(c, d_in, n, k, rPos, eps, d_nrm, d_knn))) return rc;
  HIPCHK(hipMemcpyAsync(normals_out, d_nrm, 3 * n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (knn_out) HIPCHK(hipMemcpyAsync(knn_out, d_knn, n * (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return TDTK_OK;
}

int tdtk_normals_adaptive_apx_knn(const double* xyz, size_t n, int kmin, int kmax, const double rPos[3], double eps,
                                  int device, double* normals_out, int32_t* k_used, int32_t* knn_out)
{
  int rc;
  if ((rc = adaptive_check_args(xyz, n, kmin, kmax, rPos, normals_out))) return rc;
  if (kmax > 31) { set_error("kmax + 1 = " + std::to_string((long long)kmax + 1) + " exceeds the supported list capacity of 32"); return TDTK_EUNSUP; }
  if ((rc = normals_check_args(n, kmax + 1, rPos, eps))) return rc;     // kmax + 1 > n, eps, the size of the scan
  Ctx* c;
  if ((rc = get_ctx(device, &c))) return rc;
  hipStream_t s = c->stream;
  const size_t L = knn_out ? n * (size_t)(kmax + 1) : 0;       // WS_IDX: the lists | k_used
  if ((rc = c->ws[WS_TMPA].ensure(6 * n * sizeof(double)))) return rc;   // points in | normals out
  if ((rc = c->ws[WS_IDX].ensure((L + n) * sizeof(int32_t)))) return rc;
  double* d_in = c->ws[WS_TMPA].as<double>();
  double* d_nrm = d_in + 3 * n;
  int32_t* d_knn = knn_out ? c->ws[WS_IDX].as<int32_t>() : nullptr;
  int32_t* d_k = k_used ? c->ws[WS_IDX].as<int32_t>() + L : nullptr;
  HIPCHK(hipMemcpyAsync(d_in, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, s));
  AnnTreeDev t;
  if ((rc = ann_tree_on_device(c, d_in, n, t))) return rc;
  HIPCHK(launch_ann_adaptive(t.nodes, t.root_ref, t.pts, n, kmin, kmax, eps, t.d_bb, rPos, c->ws[WS_OVF_REF].as<uint32_t>(),
                             c->ws[WS_OVF_M2].as<double>(), d_nrm, d_k, d_knn, s));
  HIPCHK(hipMemcpyAsync(normals_out, d_nrm, 3 * n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (k_used) HIPCHK(hipMemcpyAsync(k_used, d_k, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (knn_out) HIPCHK(hipMemcpyAsync(knn_out, d_knn, L * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return TDTK_OK;
}

int tdtk_scan_calc_normals(tdtk_scan* sc, int k, const double rPos[3], double eps)
{
  if (!sc) { set_error("NULL argument"); return TDTK_EINVAL; }
  int rc;
  if ((rc = normals_check_args(sc->N, k, rPos, eps))) return rc;
  Ctx* c;
  if ((rc = get_ctx(sc->device, &c))) return rc;
  hipStream_t s = c->stream;
  const size_t n = sc->N;
  if ((rc = c->ws[WS_TMPA].ensure(6 * n * sizeof(double)))) return rc;
  double* d_in = c->ws[WS_TMPA].as<double>();
  double* d_nrm = d_in + 3 * n;
  if ((rc = scan_settle(c, sc))) return rc;
  // the resident points back in the caller's order, the normals back into the resident order
  HIPCHK(launch_unsort_aos(sc->x, sc->y, sc->z, sc->d_order, n, d_in, s));
  if ((rc = normals_on_device(c, d_in, n, k, rPos, eps, d_nrm, nullptr))) return rc;
  if (!sc->nx) {
    HIPCHK(handle_malloc((void**)&sc->nx, n * sizeof(double)));
    HIPCHK(handle_malloc((void**)&sc->ny, n * sizeof(double)));
    HIPCHK(handle_malloc((void**)&sc->nz, n * sizeof(double)));
  }
  HIPCHK(launch_gather_soa(d_nrm, reinterpret_cast<const uint32_t*>(sc->d_order), n, sc->nx, sc->ny, sc->nz, s));
  HIPCHK(hipStreamSynchronize(s));
  return TDTK_OK;
}

}  // extern "C"
