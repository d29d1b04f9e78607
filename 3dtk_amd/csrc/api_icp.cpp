// icp6D::match on a resident scan: the stepped loop over scan_pass (api_search.cpp) -- or over another search tree's pass
// (icp_match_loop; the octree's is in api_octree.cpp) --, its index hashes and -R keep-masks, and the lab library's loop without
// the host in it.
#include "api_internal.h"

using namespace tdtk;

extern "C" {

// ---- icp6D::match -----------------------------------------------------------------------------
// Diagnostics (off by default): while on, every pass of tdtk_icp_match also hashes its correspondences on the device (k_idx_hash:
// the K5 hash of SURVEY 8(c) over the caller-order index array) -- the loop's indices can then be compared with a CPU run of the reference's search
// iteration by iteration at sizes where downloading a million indices per iteration is not an option.
constexpr int ICP_HASH_CAP = 1024;
int tdtk_icp_index_hashes(int on)
{
  if (on < 0) return g_icp_hashes.load(std::memory_order_relaxed);     // a question, not a switch
  return g_icp_hashes.exchange(on ? 1 : 0);
}
int tdtk_icp_last_hashes(uint64_t* out, int cap, int* n_out)
{
  if (!n_out || (cap > 0 && !out) || cap < 0) { set_error("bad argument"); return TDTK_EINVAL; }
  const int n = (int)std::min<size_t>(t_last_hashes.size(), (size_t)cap);
  for (int i = 0; i < n; i++) out[i] = t_last_hashes[(size_t)i];
  *n_out = (int)t_last_hashes.size();
  return TDTK_OK;
}

// One -R pass's keep-mask (searchTree.cc:116-118: `if (rnd > 1 && rand(rnd) != 0) continue;` for i = 0 .. N-1): one std::rand()
// per point in the caller's index order, drawn here, now -- never ahead of the pass that uses it, so the process's random
// stream is consumed exactly as a serial build of the reference consumes it (SURVEY N-d) -- and sent as N / 8 bytes; a
// small kernel turns it into one byte per query at its sorted position, which the search kernels read (SearchArgs::skip).
static int draw_keep_mask(Ctx* c, const tdtk_scan* data, int rnd, const unsigned char** skip_out)
{
  const size_t N = data->N, nbytes = (N + 7) / 8;
  int rc;
  if ((rc = c->d_mask.ensure(nbytes + 16)) || (rc = c->d_skip.ensure(N + 16))) return rc;
  c->h_mask.assign(nbytes, 0);
  for (size_t i = 0; i < N; i++) {
    const int r = (int)((double)rnd * (double)std::rand() / (RAND_MAX + 1.0));     // globals.icc:607-610
    if (r == 0) c->h_mask[i >> 3] |= (unsigned char)(1u << (i & 7u));
  }
  void* staged = nullptr;
  // (the staging buffer is reused by the next pass's mask: the copy below has been consumed by then -- every pass ends with a wait)
  if ((rc = stage_pinned(c, c->h_mask.data(), nbytes, &staged))) return rc;
  HIPCHK(hipMemcpyAsync(c->d_mask.p, staged, nbytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(launch_skip_from_mask(c->d_mask.as<unsigned char>(), data->d_order, N, c->d_skip.as<unsigned char>(), c->stream));
  *skip_out = c->d_skip.as<unsigned char>();
  return TDTK_OK;
}

#ifdef TDTK_LAB
// ---- lab: the ICP loop without the host in it (loop_dev.h; round 6, a measured negative: NEGATIVES.md) -----------------------
// For the batches of the four-lanes-per-query kernel (a real scan after -r reduction: tens of thousands of points) an
// iteration is two short kernels and a host round trip that costs as much as either.  Here the host only FEEDS the stream:
// launch k searches for iteration k after its every workgroup has made iteration k-1's solve for itself (kernels.hip:
// loop_prologue); `ahead` launches are enqueued beyond the one whose row the host is waiting for, and the host follows the
// rows of the record in pinned memory, topping the queue up.  Launches still queued when the loop ends see the flag and return
// at once.  -a 1 (QUAT), closest-point pairing, no -R, no diagnostics, at most 512 rows of pair sums (~32K points); everything
// else keeps the stepped loop below.  TDTK_ICP_DEVICE_LOOP=1 switches it on (lab library only).
constexpr int ICP_LOOP_RING = 64;
static int icp_loop_ahead()          // (read per match: a getenv is nothing beside a match, and tests flip it)
{
  const char* on = getenv("TDTK_ICP_DEVICE_LOOP");
  if (!(on && on[0] == '1')) return 0;
  const char* e = lab_env("TDTK_LOOP_AHEAD");
  const int a = e ? atoi(e) : 3;
  return std::max(1, std::min(ICP_LOOP_RING / 2, a));
}
struct IcpLoopOut {
  int iter = 0;                    // rows consumed = iterations whose solve the host has seen
  bool finished = false;           // the loop ended on the device (converged / last iteration / too few pairs)
  bool few_pairs = false;
  bool need_host = false;          // iteration `iter`'s sums are in acc / shift: the host solves it and carries on stepping
  int converged = 0;
  double ret = 0.0, prev_ret = 0.0;
  bool have_pending = false;
  double pend[16];
  double acc[ACC_TOTAL], shift[3];
};
static hipError_t await_row(const double* row, hipStream_t s)
{
  const volatile uint64_t* w = reinterpret_cast<const volatile uint64_t*>(row + ICP_ROW_READY);
  const auto t0 = std::chrono::steady_clock::now();
  bool yielding = false;
  for (uint32_t spins = 1;; spins++) {
    if (*w != SUMS_ARMED) { std::atomic_thread_fence(std::memory_order_acquire); return hipSuccess; }
    if (yielding) {
      sched_yield();
      if ((spins & 0x3Fu) != 0) continue;
    } else {
      __builtin_ia32_pause();
      if ((spins & 0x3Fu) == 0 &&
          std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > 200.0) yielding = true;
      if ((spins & 0x3FFu) != 0) continue;
    }
    const hipError_t q = hipStreamQuery(s);
    if (q == hipSuccess) return (*w != SUMS_ARMED) ? hipSuccess : hipErrorUnknown;   // (drained and the row never came)
    if (q != hipErrorNotReady) return q;
  }
}
// the loop's device block at its start: history and flags zero, the record's ring named and armed
static int icp_loop_reset(Ctx* c)
{
  int rc;
  if ((rc = c->d_loop.ensure(sizeof(IcpLoopDev)))) return rc;
  if (!c->h_loop) HIPCHK(hipHostMalloc((void**)&c->h_loop, sizeof(double) * ICP_ROW * ICP_LOOP_RING + sizeof(IcpLoopDev), hipHostMallocCoherent));
  for (int r = 0; r < ICP_LOOP_RING; r++)
    reinterpret_cast<volatile uint64_t*>(c->h_loop + (size_t)r * ICP_ROW)[ICP_ROW_READY] = SUMS_ARMED;
  IcpLoopDev* init = reinterpret_cast<IcpLoopDev*>(c->h_loop + (size_t)ICP_ROW * ICP_LOOP_RING);    // (pinned: behind the ring)
  std::memset(init, 0, sizeof *init);
  init->rows_host = c->h_loop;
  init->row_cap = ICP_LOOP_RING;
  HIPCHK(hipMemcpyAsync(c->d_loop.p, init, sizeof *init, hipMemcpyHostToDevice, c->stream));
  return TDTK_OK;
}
static int icp_device_loop(Ctx* c, const tdtk_tree* model, const double* A16, tdtk_scan* data, const tdtk_icp_params* prm,
                           bool warm_ok, double* data_transMat, double* data_dalignxf, tdtk_icp_result* res, double* trace,
                           int trace_cap, IcpLoopOut& o)
{
  hipStream_t s = c->stream;
  const size_t N = data->N;
  const int ahead = icp_loop_ahead(), max_iter = prm->max_num_iterations;
  int rc;
  if ((rc = c->ws[WS_KPOS].ensure(N * sizeof(int)))) return rc;
  const uint32_t rows = search_fused_rows(N);
  const size_t pstride = (size_t)rows * ICP_LOOP_COLS;    // two buffers of rows ([column][row]): launch k writes buffer k & 1, reads the other
  if ((rc = c->ws[WS_PART].ensure(2 * pstride * sizeof(double)))) return rc;
  if ((rc = icp_loop_reset(c))) return rc;
  Mat4 A, inv;
  std::memcpy(A.m, A16, sizeof A.m);
  m4inv(A16, inv.m);  // searchTree.cc:110
  double sh[3];
  pass_shift(model, A16, sh);
  SearchArgs sa0{};
  sa0.x = data->x; sa0.y = data->y; sa0.z = data->z;
  sa0.nx = data->nx; sa0.ny = data->ny; sa0.nz = data->nz;
  sa0.n = N;
  sa0.inv = inv; sa0.has_inv = 1;
  sa0.maxd2 = prm->max_dist_match2;
  sa0.kpos = c->ws[WS_KPOS].as<int>();
  sa0.fuse = 4; sa0.A = A;
  for (int k = 0; k < 3; k++) sa0.shift[k] = sh[k];
  sa0.loop = c->d_loop.as<IcpLoopDev>();
  sa0.loop_rows = (int)rows; sa0.loop_max_iter = max_iter; sa0.loop_eps = prm->epsilon_icp;
  const double margin = search_margin(model, prm->max_dist_match2);
  double* const P = c->ws[WS_PART].as<double>();
  // Launch k searches for iteration k; its prologue makes iteration k-1's solve and writes that iteration's row.  Launch
  // max_iter exists for its prologue alone (the last iteration's solve ends the loop before anything is searched).
  int enq = 0;
  for (;;) {
    while (enq <= max_iter && enq < o.iter + 1 + ahead) {
      SearchArgs sa = sa0;
      sa.loop_iter = enq;
      sa.partials = P + (size_t)(enq & 1) * pstride;
      sa.loop_prev = P + (size_t)((enq + 1) & 1) * pstride;
      sa.warm = (enq > 0 && warm_ok) ? 1 : 0;   // WS_KPOS holds the previous pass's hits by the time this launch runs
      sa.margin = sa.warm ? margin : 0.0;
      if ((rc = run_search(c, model, sa, 0, false, s, false))) return rc;
      enq++;
    }
    double* row = c->h_loop + (size_t)(o.iter % ICP_LOOP_RING) * ICP_ROW;
    HIPCHK(await_row(row, s));
    const int status = (int)row[ICP_ROW_STATUS];
    const uint64_t n = (uint64_t)(row[ICP_ROW_N] + 0.5);
    res->last_pairs = n;
    // (either way launch o.iter has searched, i.e. it has applied the transform of the row before: nothing is pending)
    if (status == ICP_ROW_FEW_PAIRS) { o.finished = true; o.few_pairs = true; o.have_pending = false; break; }
    if (status == ICP_ROW_NEED_HOST) {
      o.have_pending = false;
      std::memset(o.acc, 0, sizeof o.acc);
      std::memcpy(o.acc, row + ICP_ROW_ACC, ICP_LOOP_COLS * sizeof(double));
      for (int k = 0; k < 3; k++) o.shift[k] = sh[k];
      o.need_host = true;
      break;
    }
    const double ret = row[ICP_ROW_RMS];
    const double* alignxf = row + ICP_ROW_XF;
    if (!prm->quiet) std::printf("QUAT RMS point-to-point error = %10.7f  using %6llu points\n", ret, (unsigned long long)n);
    if (trace && o.iter < trace_cap) {
      double* tr = trace + (size_t)o.iter * 18;
      tr[0] = (double)n; tr[1] = ret;
      std::memcpy(tr + 2, alignxf, 16 * sizeof(double));
    }
    res->last_rms = ret;
    o.prev_ret = o.ret; o.ret = ret;
    std::memcpy(o.pend, alignxf, sizeof o.pend);
    o.have_pending = true;
    if (data_transMat) mmult(alignxf, data_transMat, data_transMat);  // scan.cc:878-898
    if (data_dalignxf) mmult(alignxf, data_dalignxf, data_dalignxf);
    reinterpret_cast<volatile uint64_t*>(row)[ICP_ROW_READY] = SUMS_ARMED;     // the ring: this slot's next turn
    if (status == ICP_ROW_CONVERGED || status == ICP_ROW_LAST) {
      o.converged = status == ICP_ROW_CONVERGED ? 1 : 0;
      o.finished = true;
      break;                       // (o.iter stays the index of this iteration: what icp6D::match returns)
    }
    o.iter++;
  }
  return TDTK_OK;
}

extern "C" int tdtk_lab_icp_device_solve(int device, const double acc17[17], const double shift[3], double alignxf[16], double* rms, int* status)
{
  if (!acc17 || !shift || !alignxf || !rms || !status) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(device, &c);
  if (rc) return rc;
  hipStream_t s = c->stream;
  if ((rc = c->ws[WS_PART].ensure(ACC_TOTAL * sizeof(double)))) return rc;
  double rowv[ACC_TOTAL] = {0.0};
  std::memcpy(rowv, acc17, ICP_LOOP_COLS * sizeof(double));
  HIPCHK(hipMemcpyAsync(c->ws[WS_PART].p, rowv, sizeof rowv, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));                      // (rowv is pageable: the copy has read it)
  if ((rc = icp_loop_reset(c))) return rc;
  HIPCHK(launch_solve_once(c->ws[WS_PART].as<double>(), 1, shift, c->d_loop.as<IcpLoopDev>(), s));
  HIPCHK(hipStreamSynchronize(s));
  const double* row = c->h_loop;
  std::memcpy(alignxf, row + ICP_ROW_XF, 16 * sizeof(double));
  *rms = row[ICP_ROW_RMS];
  *status = (int)row[ICP_ROW_STATUS];
  return TDTK_OK;
}
#endif

}  // extern "C"

// The loop of both search trees.  other == nullptr: the k-d tree `model` (tdtk_icp_match, tdtk_icp_match_rnd), every pass a
// scan_pass; else the passes are other->pass (api_internal.h) and nothing of the k-d walk's state -- warm start, certificates,
// cost order, the lab's device loop -- is used or left behind.
int tdtk::icp_match_loop(const tdtk_tree* model, const IcpTreePass* other, const double model_dalignxf[16], tdtk_scan* data,
                         double data_transMat[16], double data_dalignxf[16], const tdtk_icp_params* prm, int rnd,
                         tdtk_icp_result* res, double* trace, int trace_cap)
{
  if (!model || !model_dalignxf || !data || !prm || !res) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (prm->max_dist_match2 < 0.0 || prm->max_num_iterations < 0) {
    set_error("ERROR [ICP6D]: max_dist_match and max_num_iterations have to be >= 0");  // icp6D.cc:67-78
    return TDTK_EINVAL;
  }
  const int algo = prm->algo;
  if (algo < TDTK_ALGO_QUAT || algo > TDTK_ALGO_NAPX) {
    set_error("This minimization algorithm is not implemented");
    return TDTK_EINVAL;
  }
  const bool serial_only = algo == TDTK_ALGO_ORTHO || algo == TDTK_ALGO_DUAL || algo == TDTK_ALGO_HELIX ||
                           algo == TDTK_ALGO_LUMEULER || algo == TDTK_ALGO_LUMQUAT || algo == TDTK_ALGO_QUAT_SCALE;
  if ((algo == TDTK_ALGO_LUMEULER || algo == TDTK_ALGO_LUMQUAT) && !data_transMat) {
    set_error("LUMEULER / LUMQUAT need the current scan's transMat");
    return TDTK_EINVAL;
  }
  const int pmode = prm->pairing_mode;
  if ((pmode != 0 || algo == TDTK_ALGO_NAPX) && !data->nx) { set_error("normals required"); return TDTK_EINVAL; }
  int rc;
  if (other && (rc = other->check(pmode, prm->max_dist_match2))) return rc;
  Ctx* c;
  if ((rc = get_ctx(model->device, &c))) return rc;
  std::memset(res, 0, sizeof *res);
  if (prm->max_num_iterations == 0 || data->N == 0) return TDTK_OK;  // icp6D.cc:112-114

  if ((rc = scan_settle(c, data))) return rc;          // queued moves first: "original" and the loop both start from them
  if ((rc = scan_keep_original(c, data))) return rc;   // the loop moves the scan in place
  const unsigned want = (algo == TDTK_ALGO_APX) ? TDTK_WANT_APX
                        : (algo == TDTK_ALGO_NAPX ? TDTK_WANT_NAPX : (serial_only ? TDTK_WANT_MOM2 : 0u));
  double ret = 0.0, prev_ret = 0.0, prev_prev_ret = 0.0;
  double alignxf[16], pend[16];
  bool have_pending = false;
  double nn_total = 0.0, sums_total = 0.0;
  const double t0 = now_ms();
  int iter = 0;
  int converged = 0;
  const char* warm_env = lab_env("TDTK_WARM_START");
  const bool warm_ok = !(warm_env && warm_env[0] == '0');
  const bool hashing = g_icp_hashes.load(std::memory_order_relaxed) != 0;
  c->last_hashes.clear();
  t_last_hashes.clear();
  if (hashing) {
    if ((rc = c->d_hash.ensure(ICP_HASH_CAP * sizeof(unsigned long long)))) return rc;
    HIPCHK(hipMemsetAsync(c->d_hash.p, 0, ICP_HASH_CAP * sizeof(unsigned long long), c->stream));
  }
  bool loop_done = false, resume_with_acc = false;
  double acc[ACC_TOTAL], shift[3];
  // certificates live from one pass of THIS loop to the next (scan_pass); TDTK_CERT_SKIP=0: none (read per match, tests flip it)
  c->cert_live = false;
  const bool cert_ok = [] { const char* e = getenv("TDTK_CERT_SKIP"); return !(e && e[0] == '0'); }();
#ifdef TDTK_LAB
  // lab: the small-scan loop that runs without the host (see icp_device_loop): -a 1, closest points, every point a candidate
  if (!other && icp_loop_ahead() > 0 && algo == TDTK_ALGO_QUAT && pmode == 0 && want == 0u && rnd <= 1 && !hashing && !c->counting &&
      !kernel_timing() && fuse_mode(data->N) == 4 && search_multi_class(data->N) == 10 && search_fused_rows(data->N) <= (uint32_t)ICP_LOOP_MAX_ROWS) {
    IcpLoopOut o;
    if ((rc = icp_device_loop(c, model, model_dalignxf, data, prm, warm_ok, data_transMat, data_dalignxf, res, trace, trace_cap, o))) return rc;
    iter = o.iter;
    ret = o.ret; prev_ret = o.prev_ret;
    have_pending = o.have_pending;
    if (have_pending) std::memcpy(pend, o.pend, sizeof pend);
    converged = o.converged;
    loop_done = o.finished;
    if (o.need_host) {             // a solve that did not come out finite on the device: this iteration's sums, the host's solver
      std::memcpy(acc, o.acc, sizeof acc);
      for (int k = 0; k < 3; k++) shift[k] = o.shift[k];
      resume_with_acc = true;
      // (the launches still queued behind the failed solve return at once: the flag is up; the stepped loop below takes over)
    }
  }
#endif
  for (; !loop_done && iter < prm->max_num_iterations; iter++) {
    prev_prev_ret = prev_ret;
    prev_ret = ret;
    // -R: this pass's candidates (drawn now, in the reference's order)
    const unsigned char* skip = nullptr;
    if (rnd > 1 && (rc = draw_keep_mask(c, data, rnd, &skip))) return rc;
    // the previous iteration's alignxf is applied to the points inside the search kernel
    // (the warm start stays exact under -R: WS_KPOS holds -1 for whoever was not drawn last time -- a cold start --, and for
    // the others a point of THIS tree, whose distance bounds the nearest neighbour's however the scan has moved since)
    if (!resume_with_acc) {
      if (other) {
        rc = other->pass(have_pending ? pend : nullptr, skip, want, acc, shift);
        if (rc) res->iterations = iter;      // (the scan and the matrices hold the iterations before this one, all of them)
      } else {
        rc = scan_pass(c, model, model_dalignxf, data, pmode, prm->max_dist_match2, want, nullptr,
                       have_pending ? pend : nullptr, true, acc, shift, iter > 0 && warm_ok, skip,
                       cert_ok && iter > 0 && rnd <= 1);
      }
      if (rc) return rc;
      have_pending = false;
    }
    resume_with_acc = false;
    if (hashing && iter < ICP_HASH_CAP)    // this pass's correspondences are still in the workspace (sorted positions)
      HIPCHK(launch_idx_hash(c->ws[WS_KPOS].as<int>(), data->d_order, model->dev.pts, data->N,
                             c->d_hash.as<unsigned long long>() + iter, c->stream));
    double ms = 0, sms = 0;
    collect_ms(c, &ms, &sms);
    nn_total += ms;
    sums_total += sms;
    tdtk_pair_sums sums;
    finish_sums(acc, shift, data->N, want, &sums);
    res->last_pairs = sums.n;
    if (sums.n > 3) {  // icp6D.cc:235-243 (serial branch semantics)
      std::string err;
      double rms = 0;
      // getAlgorithmID() 3 / 8: alignxf enters as CurrentScan->get_transMat() (icp6D.cc:237-241)
      if (data_transMat) std::memcpy(alignxf, data_transMat, sizeof alignxf);
      rc = align_from_sums(algo, sums, alignxf, &rms, err);
      if (rc == TDTK_ESOLVE) {
        // the reference prints and keeps going with ret = -1 and the unchanged alignxf buffer
        ret = -1.0;
        m4identity(alignxf);
      } else if (rc) { set_error(err); return rc; }
      else ret = rms;
    } else {
      break;
    }
    if (!prm->quiet) {
      static const char* tag[] = {"", "QUAT", "SVD", "ORTHO", "DUALQUAT", "HELIX", "APX", "LUMEULER", "LUMQUAT",
                                  "QUAT SCALE", "APX"};
      std::printf("%s RMS point-to-%s error = %10.7f  using %6llu points\n", tag[algo],
                  algo == TDTK_ALGO_NAPX ? "plane" : "point", ret, (unsigned long long)sums.n);
    }
    if (trace && iter < trace_cap) {
      double* row = trace + (size_t)iter * 18;
      row[0] = (double)sums.n; row[1] = ret;
      std::memcpy(row + 2, alignxf, sizeof alignxf);
    }
    res->last_rms = ret;
    // CurrentScan->transform(alignxf, ...): points lazily (next search or epilogue), matrices now
    std::memcpy(pend, alignxf, sizeof pend);
    have_pending = true;
    if (data_transMat) mmult(alignxf, data_transMat, data_transMat);  // scan.cc:878-898
    if (data_dalignxf) mmult(alignxf, data_dalignxf, data_dalignxf);
    if ((std::fabs(ret - prev_ret) < prm->epsilon_icp && std::fabs(ret - prev_prev_ret) < prm->epsilon_icp) ||
        iter == prm->max_num_iterations - 1) {
      converged = (iter != prm->max_num_iterations - 1) ? 1 : 0;
      break;
    }
  }
  if (have_pending) {
    Mat4 P;
    std::memcpy(P.m, pend, sizeof P.m);
    HIPCHK(launch_transform(data->x, data->y, data->z, data->nx, data->ny, data->nz, data->N, P, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  if (hashing) {
    const int passes = std::min(ICP_HASH_CAP, std::min(iter + 1, prm->max_num_iterations));
    c->last_hashes.assign((size_t)passes, 0);
    HIPCHK(hipMemcpyAsync(c->last_hashes.data(), c->d_hash.p, (size_t)passes * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    t_last_hashes = c->last_hashes;
  }
  res->iterations = iter;
  res->converged = converged;
  res->total_ms = now_ms() - t0;
  res->nn_ms = nn_total;
  res->sums_ms = sums_total;
  if (!prm->quiet) std::printf("TIME  %ld   ITER %d\n", (long)res->total_ms, iter);
  return TDTK_OK;
}

extern "C" {

int tdtk_icp_match(const tdtk_tree* model, const double model_dalignxf[16], tdtk_scan* data,
                   double data_transMat[16], double data_dalignxf[16], const tdtk_icp_params* prm,
                   tdtk_icp_result* res, double* trace, int trace_cap)
{
  return icp_match_loop(model, nullptr, model_dalignxf, data, data_transMat, data_dalignxf, prm, 1, res, trace, trace_cap);
}
int tdtk_icp_match_rnd(const tdtk_tree* model, const double model_dalignxf[16], tdtk_scan* data,
                       double data_transMat[16], double data_dalignxf[16], const tdtk_icp_params* prm, int rnd,
                       tdtk_icp_result* res, double* trace, int trace_cap)
{
  return icp_match_loop(model, nullptr, model_dalignxf, data, data_transMat, data_dalignxf, prm, rnd, res, trace, trace_cap);
}

}  // extern "C"
