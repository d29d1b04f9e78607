// The resident scan handle: the tdtk_scan_* entry points, one pass of pairs and sums over a scan (tdtk_scan_pairs,
// tdtk_point_point_error, tdtk_get_pt_pairs) and the batched moves of many scans.
#include "api_internal.h"

using namespace tdtk;

extern "C" {

// ---- resident scan ---------------------------------------------------------------------
int tdtk_scan_create(const double* xyz, const double* nrm, size_t N, int device, tdtk_scan** out)
{
  if (!out) { set_error("out is NULL"); return TDTK_EINVAL; }
  *out = nullptr;
  if (!xyz && N) { set_error("NULL points"); return TDTK_EINVAL; }
  if (N >= (1ull << 32)) { set_error("scan too large"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(device, &c);
  if (rc) return rc;
  std::unique_ptr<tdtk_scan> sc(new tdtk_scan);
  sc->device = device; sc->N = N;
  if (N == 0) { *out = sc.release(); return TDTK_OK; }
  hipStream_t s = c->stream;
  const size_t tmp_bytes = morton_sort_temp_bytes(N);
  if ((rc = c->ws[WS_TMPA].ensure(3 * N * sizeof(double)))) return rc;        // AoS staging
  if ((rc = c->ws[WS_CELL].ensure(2 * N * sizeof(uint32_t)))) return rc;      // keys a|b
  if ((rc = c->ws[WS_ORDER].ensure(N * sizeof(uint32_t)))) return rc;         // idx a
  if ((rc = c->ws[WS_TMPB].ensure(tmp_bytes + 256))) return rc;
  if ((rc = c->ws[WS_BOX].ensure(bbox_temp_bytes() + 8 * sizeof(double)))) return rc;
  double* d_box = c->ws[WS_BOX].as<double>();
  double* d_aos = c->ws[WS_TMPA].as<double>();
  uint32_t* keys_a = c->ws[WS_CELL].as<uint32_t>();
  uint32_t* keys_b = keys_a + N;
  uint32_t* idx_a = c->ws[WS_ORDER].as<uint32_t>();
  HIPCHK(handle_malloc((void**)&sc->d_order, N * sizeof(int32_t)));
  HIPCHK(handle_malloc((void**)&sc->x, N * sizeof(double)));
  HIPCHK(handle_malloc((void**)&sc->y, N * sizeof(double)));
  HIPCHK(handle_malloc((void**)&sc->z, N * sizeof(double)));
  HIPCHK(hipMemcpyAsync(d_aos, xyz, 3 * N * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(launch_bbox(d_aos, N, d_box + 8, d_box, s));
  HIPCHK(launch_morton_order(d_aos, N, d_box, keys_a, idx_a, keys_b, reinterpret_cast<uint32_t*>(sc->d_order),
                             c->ws[WS_TMPB].p, tmp_bytes, s));
  HIPCHK(launch_gather_soa(d_aos, reinterpret_cast<const uint32_t*>(sc->d_order), N, sc->x, sc->y, sc->z, s));
  if (nrm) {
    HIPCHK(handle_malloc((void**)&sc->nx, N * sizeof(double)));
    HIPCHK(handle_malloc((void**)&sc->ny, N * sizeof(double)));
    HIPCHK(handle_malloc((void**)&sc->nz, N * sizeof(double)));
    HIPCHK(hipMemcpyAsync(d_aos, nrm, 3 * N * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(launch_gather_soa(d_aos, reinterpret_cast<const uint32_t*>(sc->d_order), N, sc->nx, sc->ny, sc->nz, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  *out = sc.release();
  return TDTK_OK;
}

void tdtk_scan_destroy(tdtk_scan* s)
{
  if (!s) return;
  wait_deferred(s->device);   // a deferred k_transform2_batch may still be writing this scan's arrays
  delete s;   // ~tdtk_scan releases the device arrays
}

size_t tdtk_scan_size(const tdtk_scan* s) { return s ? s->N : 0; }

int tdtk_scan_transform(tdtk_scan* s, const double alignxf[16])
{
  if (!s || !alignxf) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(s->device, &c);
  if (rc) return rc;
  if ((rc = scan_keep_original(c, s))) return rc;
  std::unique_lock<std::recursive_mutex> lk(g_moves_mu);
  if (!s->pending.empty()) {
    // behind moves that are still queued: this one joins the queue (order is what matters)
    scan_queue_move(s, alignxf);
    if (!lazy_moves() || s->pending.size() >= LAZY_CHAIN_MAX) {
      if ((rc = scan_settle(c, s))) return rc;
      HIPCHK(hipStreamSynchronize(c->stream));
    }
    return TDTK_OK;
  }
  lk.unlock();
  Mat4 A;
  std::memcpy(A.m, alignxf, sizeof A.m);
  HIPCHK(launch_transform(s->x, s->y, s->z, s->nx, s->ny, s->nz, s->N, A, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TDTK_OK;
}

static int scan_to_host(Ctx* c, const tdtk_scan* s, const double* x, const double* y, const double* z, double* out);

int tdtk_scan_mark_original(tdtk_scan* s)
{
  if (!s) { set_error("NULL argument"); return TDTK_EINVAL; }
  (void)hipSetDevice(s->device);
  wait_deferred(s->device);   // the saved original may be in use by a move that was left running
  if (s->npend.load(std::memory_order_acquire) != 0) {  // "original" = the points as they are now, queued moves included
    Ctx* c;
    int rc = get_ctx(s->device, &c);
    if (rc) return rc;
    if ((rc = scan_settle(c, s))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  double* p[] = {s->ox, s->oy, s->oz};
  for (double* q : p)
    if (q) pool_free(q);
  s->ox = s->oy = s->oz = nullptr;
  s->track_original = true;
  return TDTK_OK;
}

int tdtk_scan_download_original(const tdtk_scan* s, double* xyz_out)
{
  if (!s || !xyz_out) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(s->device, &c);
  if (rc) return rc;
  if (!s->ox && (rc = scan_settle(c, s))) return rc;
  return scan_to_host(c, s, s->ox ? s->ox : s->x, s->ox ? s->oy : s->y, s->ox ? s->oz : s->z, xyz_out);
}

// sorted SoA -> caller-order AoS on the device, then one contiguous copy to the host
static int scan_to_host(Ctx* c, const tdtk_scan* s, const double* x, const double* y, const double* z, double* out)
{
  const size_t N = s->N;
  if (!N) return TDTK_OK;
  int rc = c->ws[WS_TMPA].ensure(3 * N * sizeof(double));
  if (rc) return rc;
  HIPCHK(launch_unsort_aos(x, y, z, s->d_order, N, c->ws[WS_TMPA].as<double>(), c->stream));
  HIPCHK(hipMemcpyAsync(out, c->ws[WS_TMPA].p, 3 * N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TDTK_OK;
}

int tdtk_scan_download(const tdtk_scan* s, double* xyz_out, double* nrm_out)
{
  if (!s || !xyz_out) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(s->device, &c);
  if (rc) return rc;
  if ((rc = scan_settle(c, s))) return rc;
  if ((rc = scan_to_host(c, s, s->x, s->y, s->z, xyz_out))) return rc;
  if (nrm_out && s->nx) rc = scan_to_host(c, s, s->nx, s->ny, s->nz, nrm_out);
  return rc;
}

int tdtk_scan_pairs(const tdtk_tree* model, const double A[16], tdtk_scan* data, int pmode, double maxd2,
                    uint32_t want, const double* lum_D, int32_t* idx_out, tdtk_pair_sums* sums)
{
  if (!model || !A || !data || !sums) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (pmode < 0 || pmode > 2) { set_error("bad pairing mode"); return TDTK_EINVAL; }
  if ((pmode != 0 || (want & TDTK_WANT_NAPX)) && data->N && !data->nx) {   // an empty scan pairs with nothing
    set_error("this pairing mode / minimizer needs normals");
    return TDTK_EINVAL;
  }
  if (model->device != data->device) { set_error("tree and scan live on different devices"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(model->device, &c);
  if (rc) return rc;
  std::memset(sums, 0, sizeof *sums);
  sums->n_queries = data->N;
  if (data->N == 0) return TDTK_OK;
  double acc[ACC_TOTAL], shift[3];
  rc = scan_pass(c, model, A, data, pmode, maxd2, want, lum_D, nullptr, true, acc, shift);
  if (rc) return rc;
  finish_sums(acc, shift, data->N, want, sums);
  if (lum_D) sums->lum_sumd2 = acc[ACC_LSS];  // second-pass residual rides here (see tdtk_lum_link)
  if (idx_out) rc = scan_idx_to_host(c, model, data, idx_out);
  collect_ms(c, nullptr);
  return rc;
}

// icp6D::Point_Point_Error (icp6D.cc:293-367)
int tdtk_point_point_error(const tdtk_tree* model, const double A[16], tdtk_scan* data, double max_dist_match,
                           double scale_max, uint64_t* np_out, double* error_out)
{
  if (!model || !A || !data || !error_out) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (model->device != data->device) { set_error("tree and scan live on different devices"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(model->device, &c);
  if (rc) return rc;
  if (np_out) *np_out = 0;
  *error_out = 0.0;
  const size_t N = data->N;
  if (N == 0) { *error_out = std::nan(""); return TDTK_OK; }   // 0 / 0 in the reference
  hipStream_t s = c->stream;
  if ((rc = c->ws[WS_KPOS].ensure(N * sizeof(int)))) return rc;
  if ((rc = scan_settle(c, data))) return rc;
  Mat4 Am, inv;
  std::memcpy(Am.m, A, sizeof Am.m);
  m4inv(A, inv.m);
  SearchArgs sa{};
  sa.x = data->x; sa.y = data->y; sa.z = data->z;
  sa.n = N; sa.inv = inv; sa.has_inv = 1;
  sa.maxd2 = max_dist_match * max_dist_match;
  sa.kpos = c->ws[WS_KPOS].as<int>();
  if ((rc = run_search(c, model, sa, 0, false, s, true))) return rc;
  AccumArgs aa{};
  aa.T = model->dev;
  aa.x = data->x; aa.y = data->y; aa.z = data->z;
  aa.kpos = sa.kpos; aa.n = N; aa.A = Am; aa.inv = inv;
  const uint32_t grid = accum_grid(N);
  if ((rc = c->ws[WS_PART].ensure((size_t)grid * ACC_TOTAL * sizeof(double)))) return rc;
  const double scale = std::log(scale_max) / (max_dist_match * max_dist_match);   // icp6D.cc:299
  HIPCHK(launch_pp_error(aa, grid, scale, c->ws[WS_PART].as<double>(), c->h_pin, s));
  HIPCHK(hipStreamSynchronize(s));
  collect_ms(c, nullptr);
  const double se = c->h_pin[0], cn = c->h_pin[1];
  if (np_out) *np_out = (uint64_t)(cn + 0.5);
  *error_out = (-0.39894228 * se) / cn;   // error -= 0.39894228 * exp(dist * scale) per pair; error / nr_ppairs
  return TDTK_OK;
}

}  // extern "C"

namespace tdtk {

// SearchTree::getPtPairs around any tree: `t` gives the device, the leaf-ordered points (dev.pts) and the accumulation point;
// `pairs` is the whole-scan pass over the resident queries (tdtk_scan_pairs for the k-d tree, the octree's own for BOctTree)
// and leaves its hits in WS_KPOS
int get_pt_pairs_over(const tdtk_tree* t, const PairsPass& pairs, const double A[16], const double* xyz_r, const double* normal_r,
                      size_t start, size_t end, int rnd, int pmode, double maxd2, uint32_t want,
                      int32_t* idx_out, double* p1_out, double* p2_out, double* pn_out, tdtk_pair_sums* sums)
{
  if (!t || !A || !xyz_r || !sums || end < start) { set_error("bad argument"); return TDTK_EINVAL; }
  if ((pmode == 1 || pmode == 2 || (want & TDTK_WANT_NAPX)) && !normal_r) {
    set_error("this pairing mode / minimizer needs normals");
    return TDTK_EINVAL;
  }
  // rnd > 1: "take about 1/rnd-th of the numbers only" (searchTree.cc:118, globals.icc:607-610):
  // one std::rand() per candidate, consumed in index order like a serial (non-OpenMP) reference
  // build does.  The keep-mask is drawn on the host; only the kept queries go to the GPU.
  std::vector<double> kept_xyz, kept_nrm;
  std::vector<size_t> kept_pos;
  const double* q_xyz = xyz_r + 3 * start;
  const double* q_nrm = normal_r ? normal_r + 3 * start : nullptr;
  size_t n = end - start;
  const size_t n_all = n;
  if (rnd > 1) {
    for (size_t i = 0; i < n_all; i++) {
      const int r = (int)((double)rnd * (double)std::rand() / (RAND_MAX + 1.0));
      if (r != 0) continue;
      kept_pos.push_back(i);
      for (int k = 0; k < 3; k++) kept_xyz.push_back(q_xyz[3 * i + k]);
      if (q_nrm) for (int k = 0; k < 3; k++) kept_nrm.push_back(q_nrm[3 * i + k]);
    }
    n = kept_pos.size();
    q_xyz = kept_xyz.data();
    if (q_nrm) q_nrm = kept_nrm.data();
    if (idx_out) for (size_t i = 0; i < n_all; i++) idx_out[i] = -1;
  }
  tdtk_scan* sc = nullptr;
  int rc = tdtk_scan_create(q_xyz, q_nrm, n, t->device, &sc);
  if (rc) return rc;
  std::vector<int32_t> idx_local;
  int32_t* idx = nullptr;
  const bool want_pairs = p1_out || p2_out || pn_out;
  if (rnd > 1 || (!idx_out && want_pairs)) { idx_local.resize(n ? n : 1); idx = idx_local.data(); }
  else idx = idx_out;
  rc = pairs(sc, idx, sums);
  if (rc) { tdtk_scan_destroy(sc); return rc; }
  sums->n_queries = n;
  if (want_pairs && n && sums->n) {
    // the PtPair(s, t, normal) list of searchTree.cc:147-180 in query order, built on the device:
    // found flags (caller order) -> prefix sum -> one kernel writes the compact lists
    Ctx* c;
    if ((rc = get_ctx(t->device, &c))) { tdtk_scan_destroy(sc); return rc; }
    hipStream_t s = c->stream;
    const size_t np = sums->n;
    const size_t tmpb = scan_u32_temp_bytes(n + 1);
    if ((rc = c->ws[WS_CELL].ensure(2 * (n + 1) * sizeof(uint32_t))) || (rc = c->ws[WS_TMPB].ensure(tmpb + 256)) ||
        (rc = c->ws[WS_TMPA].ensure(9 * np * sizeof(double)))) { tdtk_scan_destroy(sc); return rc; }
    uint32_t* flags = c->ws[WS_CELL].as<uint32_t>();
    uint32_t* slot = flags + (n + 1);
    double* d_p1 = c->ws[WS_TMPA].as<double>();
    double* d_p2 = d_p1 + 3 * np;
    double* d_pn = d_p2 + 3 * np;
    auto bail = [&](int code) { tdtk_scan_destroy(sc); return code; };
    if (hipMemsetAsync(flags + n, 0, sizeof(uint32_t), s) != hipSuccess) return bail(TDTK_EDEVICE);
    if (launch_found_flags(c->ws[WS_KPOS].as<int>(), sc->d_order, n, flags, s) != hipSuccess) return bail(TDTK_EDEVICE);
    if (launch_scan_u32(flags, slot, n + 1, c->ws[WS_TMPB].p, tmpb, s) != hipSuccess) return bail(TDTK_EDEVICE);
    PairListArgs pa{};
    pa.T = t->dev;
    pa.x = sc->x; pa.y = sc->y; pa.z = sc->z;
    const bool use_n = sc->nx && (pmode != 0 || (want & TDTK_WANT_NAPX));
    pa.nx = use_n ? sc->nx : nullptr; pa.ny = use_n ? sc->ny : nullptr; pa.nz = use_n ? sc->nz : nullptr;
    pa.kpos = c->ws[WS_KPOS].as<int>();
    pa.order = sc->d_order; pa.slot = slot; pa.n = n;
    std::memcpy(pa.A.m, A, sizeof pa.A.m);
    m4inv(A, pa.inv.m);
    pa.p1 = p1_out ? d_p1 : nullptr; pa.p2 = p2_out ? d_p2 : nullptr; pa.pn = pn_out ? d_pn : nullptr;
    if (pn_out && !use_n && hipMemsetAsync(d_pn, 0, 3 * np * sizeof(double), s) != hipSuccess) return bail(TDTK_EDEVICE);
    if (use_n || !pn_out) { /* kernel writes pn when normals take part */ }
    else pa.pn = nullptr;
    if (launch_pair_list(pa, pmode, s) != hipSuccess) return bail(TDTK_EDEVICE);
    bool ok = true;
    if (p1_out) ok &= hipMemcpyAsync(p1_out, d_p1, 3 * np * sizeof(double), hipMemcpyDeviceToHost, s) == hipSuccess;
    if (p2_out) ok &= hipMemcpyAsync(p2_out, d_p2, 3 * np * sizeof(double), hipMemcpyDeviceToHost, s) == hipSuccess;
    if (pn_out) ok &= hipMemcpyAsync(pn_out, d_pn, 3 * np * sizeof(double), hipMemcpyDeviceToHost, s) == hipSuccess;
    ok &= hipStreamSynchronize(s) == hipSuccess;
    if (!ok) { set_error("pair list copy failed"); return bail(TDTK_EDEVICE); }
  }
  tdtk_scan_destroy(sc);
  if (rnd > 1 && idx_out)
    for (size_t i = 0; i < n; i++) idx_out[kept_pos[i]] = idx[i];
  return TDTK_OK;
}

}  // namespace tdtk

extern "C" {

int tdtk_get_pt_pairs(const tdtk_tree* t, const double A[16], const double* xyz_r, const double* normal_r,
                      size_t start, size_t end, int rnd, int pmode, double maxd2, uint32_t want,
                      const double* lum_D, int32_t* idx_out, double* p1_out, double* p2_out,
                      double* pn_out, tdtk_pair_sums* sums)
{
  const PairsPass pass = [&](tdtk_scan* sc, int32_t* idx, tdtk_pair_sums* o) { return tdtk_scan_pairs(t, A, sc, pmode, maxd2, want, lum_D, idx, o); };
  return get_pt_pairs_over(t, pass, A, xyz_r, normal_r, start, end, rnd, pmode, maxd2, want, idx_out, p1_out, p2_out, pn_out, sums);
}

}  // extern "C"

namespace tdtk {

// many resident scans moved in place by A1 and then (optionally) A2.  The moves are queued on the scans (tdtk_scan::pending)
// and carried out by whoever reads a scan next; TDTK_LAZY_MOVES=0 (or a chain that has grown long): one launch now, left
// running behind the process-wide fence.
int queue_scan_moves(Ctx* c, const std::vector<tdtk_scan*>& moved)
{
  if (moved.empty()) return TDTK_OK;
  std::vector<const tdtk_scan*> now;
  for (tdtk_scan* sc : moved)
    if (!lazy_moves() || sc->npend.load(std::memory_order_acquire) >= LAZY_CHAIN_MAX) now.push_back(sc);
  if (now.empty()) return TDTK_OK;
  int rc = scans_settle(c, now.data(), (int)now.size());
  if (rc) return rc;
  return defer_fence(c);
}

}  // namespace tdtk

extern "C" {

int tdtk_scans_transform2(int count, tdtk_scan* const* scans, const double* A1, const double* A2)
{
  if (count < 0 || (count && (!scans || !A1))) { set_error("bad argument"); return TDTK_EINVAL; }
  Ctx* c = nullptr;
  std::vector<tdtk_scan*> moved;
  for (int i = 0; i < count; i++) {
    tdtk_scan* sc = scans[i];
    if (!sc || !sc->N) continue;
    if (!c) { int rc = get_ctx(sc->device, &c); if (rc) return rc; }
    if (sc->device != c->device) { set_error("resident scans of one call must live on one device"); return TDTK_EINVAL; }
    { int rk = scan_keep_original(c, sc); if (rk) return rk; }
    scan_queue_move(sc, A1 + 16 * (size_t)i);
    if (A2) scan_queue_move(sc, A2 + 16 * (size_t)i);
    moved.push_back(sc);
  }
  if (!c) return TDTK_OK;
  return queue_scan_moves(c, moved);
}

}  // extern "C"
