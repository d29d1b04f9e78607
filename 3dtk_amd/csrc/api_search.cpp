// Closest-point search: the internals of one pass (the search launch, the pair sums and the wait for them, scan_pass -- the host
// part of an ICP iteration, kept in this one file), the tdtk_find_closest* family, the timing and visit-counter entries and
// tdtk_measure_bandwidth.
#include "api_internal.h"

using namespace tdtk;

namespace tdtk {

// ------------------------------------------------------------------------------------------
// internal: one search pass over SoA queries
// ------------------------------------------------------------------------------------------
// the spill area behind the LDS stacks: [level][lane] for as many lanes as ANY search kernel may launch for this
// batch size (every kernel indexes it with its own grid, all of them <= search_max_lanes)
int prepare_overflow_in(DevBuf& bm2, DevBuf& bref, const tdtk_tree* t, size_t nq, SearchArgs& a)
{
  const int need = (int)t->info.max_depth - 1 - search_lds_depth();
  a.ovf_m2 = nullptr; a.ovf_ref = nullptr;
  if (need > 0) {
    const size_t lanes = search_max_lanes(nq);
    int rc = bm2.ensure(lanes * need * sizeof(double));
    if (rc) return rc;
    rc = bref.ensure(lanes * need * sizeof(uint32_t));
    if (rc) return rc;
    a.ovf_m2 = bm2.as<double>();
    a.ovf_ref = bref.as<uint32_t>();
  }
  return TDTK_OK;
}
static int prepare_overflow(Ctx* c, const tdtk_tree* t, size_t nq, SearchArgs& a)
{
  return prepare_overflow_in(c->ws[WS_OVF_M2], c->ws[WS_OVF_REF], t, nq, a);
}

// HIP events around the search and the pair-sum kernels of every pass (tdtk_icp_result.nn_ms / sums_ms,
// tdtk_last_kernel_ms, tdtk_last_timings) are a profiling aid and OFF unless asked for (tdtk_kernel_timing(1) or
// TDTK_KERNEL_TIMING=1): four marker packets on the stream, two event waits and two read-outs per ICP iteration cost
// 10 us of it -- 4 % of a 1M-point iteration, 19 % of an 81K-point one (0.2602 -> 0.2504 ms, 54.9 -> 44.4 us).
bool kernel_timing()
{
  int v = g_kernel_timing.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("TDTK_KERNEL_TIMING");
    v = (e && e[0] == '1') ? 1 : 0;
    g_kernel_timing.store(v, std::memory_order_relaxed);
  }
  return v != 0;
}

int run_search(Ctx* c, const tdtk_tree* t, SearchArgs& a, int dirmode, bool count, hipStream_t s, bool timed)
{
  timed = timed && kernel_timing();
  a.T = t->dev;
  const uint32_t grid = search_grid(a.n);
  int rc = prepare_overflow(c, t, a.n, a);
  if (rc) return rc;
  if (c->counting && dirmode == 0 && !count) {
    count = true;
    a.counters = c->d_counters.as<unsigned long long>();
    c->counted_queries += a.n;
  }
  if (dirmode == 0 && search_uses_queue(a.n)) {
    if (s != c->stream) {   // the counters belong to this context's stream: order a caller's stream behind it
      HIPCHK(hipEventRecord(c->e_user, c->stream));
      HIPCHK(hipStreamWaitEvent(s, c->e_user, 0));
    }
    if ((rc = c->qc.attach(a))) return rc;
  }
  if (timed) HIPCHK(hipEventRecord(c->e0, s));
  HIPCHK(launch_search(a, grid, dirmode, count, s));
  if (timed) { HIPCHK(hipEventRecord(c->e1, s)); c->ev_pending = true; }
  return TDTK_OK;
}

int collect_ms(Ctx* c, double* ms, double* sums_ms)
{
  if (c->ev_pending) {
    HIPCHK(hipEventSynchronize(c->e1));
    float f = 0;
    HIPCHK(hipEventElapsedTime(&f, c->e0, c->e1));
    c->last_nn_ms = f;
    c->ev_pending = false;
  }
  if (c->ev2_pending) {
    HIPCHK(hipEventSynchronize(c->e3));
    float f = 0;
    HIPCHK(hipEventElapsedTime(&f, c->e2, c->e3));
    c->last_sums_ms = f;
    c->ev2_pending = false;
  }
  if (c->ev4_pending) {
    HIPCHK(hipEventSynchronize(c->e5));
    float f = 0;
    HIPCHK(hipEventElapsedTime(&f, c->e4, c->e5));
    c->last_normals_ms = f;
    c->ev4_pending = false;
  }
  const bool on = kernel_timing();
  if (ms) *ms = on ? c->last_nn_ms : 0.0;
  if (sums_ms) *sums_ms = on ? c->last_sums_ms : 0.0;
  return TDTK_OK;
}

// Retire-time accumulation inside the search kernel (kernels.hip, FUSE 1) is OFF by default: its 34 accumulator
// registers take the kernel from 7 to 4 waves per SIMD and every retire waits for its own gather, so the search
// grows by about what the separate pair-sum pass costs (1M-vs-1M ICP: 0.2881 + 0.0072 ms fused against
// 0.2708 + 0.0280 ms; 4M: 1.179 + 0.016 against 0.965 + 0.058 -- gpurun_out/r2a/sweep.log).  TDTK_FUSE_SUMS=1 selects it.
// Batches below the persistent-lane kernel's size are another matter: their kernels are not short of issue slots, and
// the workgroup sums its own chunk once it is through with it (chunk_pair_sums): an 81K-point ICP iteration is two
// launches instead of three.  On by default there, TDTK_FUSE_SUMS=0 switches it off.
int fuse_mode(size_t N)          // 0: separate k_accum, 1: at retire time, 3: by each wave after its last query,
{                                // 4: by each workgroup after its chunk (small batches)
  const char* e = lab_env("TDTK_FUSE_SUMS");
  const int v = e ? atoi(e) : -1;
  const int kind = search_fuse_kind(N);
  if (kind == 2) return v == 0 ? 0 : 4;
  // round 3: 3 is the default -- with the bucket-group kernel (four waves per SIMD either way) the waves that are done early
  // add up their own slabs while the launch waits for the slowest: 1M-vs-1M 0.2217 -> 0.2183 ms per iteration at the
  // driver's arguments, 0.2000 -> 0.1925 over 100 (the separate k_accum launch, 18-24 us, is gone; the search grows by ~10)
  if (kind == 1) return (v == 0 || v == 1 || v == 3) ? v : (search_fuse_after_last_pays(N) ? 3 : 0);   // (4M and more: k_accum)
  return 0;
}

// acc[ACC_TOTAL] (sums about `shift`) -> the reference's quantities
void finish_sums(const double* acc, const double shift[3], size_t nq, unsigned want, tdtk_pair_sums* o)
{
  std::memset(o, 0, sizeof *o);
  o->n_queries = nq;
  const double n = acc[ACC_N];
  o->n = (uint64_t)(n + 0.5);
  o->sum = acc[ACC_SUM];
  o->lum_sumd2 = acc[ACC_SUM];
  if (o->n == 0) return;
  const double* Sm = acc + ACC_SM;
  const double* Sd = acc + ACC_SD;
  double wm[3], wd[3];
  for (int a = 0; a < 3; a++) {
    wm[a] = Sm[a] / n; wd[a] = Sd[a] / n;
    o->centroid_m[a] = shift[a] + wm[a];
    o->centroid_d[a] = shift[a] + wd[a];
  }
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) o->Si[a * 3 + b] = acc[ACC_P + a * 3 + b] - Sm[a] * Sd[b] / n;
  if (want & TDTK_WANT_APX) {
    double D2[3][3], Dc[3][3], E[3][3];
    const double* dd = acc + ACC_DD;
    D2[0][0] = dd[0]; D2[0][1] = D2[1][0] = dd[1]; D2[0][2] = D2[2][0] = dd[2];
    D2[1][1] = dd[3]; D2[1][2] = D2[2][1] = dd[4]; D2[2][2] = dd[5];
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) {
        Dc[a][b] = D2[a][b] - Sd[a] * Sd[b] / n;
        // E[a][b] = sum (p1-p2)_a (p2-cd)_b
        E[a][b] = acc[ACC_P + a * 3 + b] - D2[a][b] - (Sm[a] - Sd[a]) * Sd[b] / n;
      }
    o->apx_A[0] = Dc[1][1] + Dc[2][2];
    o->apx_A[1] = -Dc[0][1];
    o->apx_A[2] = -Dc[0][2];
    o->apx_A[3] = Dc[0][0] + Dc[2][2];
    o->apx_A[4] = -Dc[1][2];
    o->apx_A[5] = Dc[0][0] + Dc[1][1];
    o->apx_B[0] = E[2][1] - E[1][2];
    o->apx_B[1] = E[0][2] - E[2][0];
    o->apx_B[2] = E[1][0] - E[0][1];
  }
  if (want & TDTK_WANT_NAPX) {
    // c_true = (p2 - cd) x n = u0 - w x n,  w = cd - shift  ->  v_true = L v0,
    // L = [[I, -W], [0, I]], W = [w]x
    double A0[6][6], L[6][6], T1[6][6];
    int q = 0;
    for (int r = 0; r < 6; r++)
      for (int s = r; s < 6; s++) { A0[r][s] = A0[s][r] = acc[ACC_NA + q]; q++; }
    for (int r = 0; r < 6; r++)
      for (int s = 0; s < 6; s++) L[r][s] = (r == s) ? 1.0 : 0.0;
    const double* w = wd;
    L[0][4] = w[2];  L[0][5] = -w[1];
    L[1][3] = -w[2]; L[1][5] = w[0];
    L[2][3] = w[1];  L[2][4] = -w[0];
    for (int r = 0; r < 6; r++)
      for (int s = 0; s < 6; s++) {
        double v = 0;
        for (int k = 0; k < 6; k++) v += L[r][k] * A0[k][s];
        T1[r][s] = v;
      }
    q = 0;
    for (int r = 0; r < 6; r++)
      for (int s = r; s < 6; s++) {
        double v = 0;
        for (int k = 0; k < 6; k++) v += T1[r][k] * L[s][k];
        o->napx_A[q++] = v;
      }
    for (int r = 0; r < 6; r++) {
      double v = 0;
      for (int k = 0; k < 6; k++) v += L[r][k] * acc[ACC_NB + k];
      o->napx_B[r] = v;
    }
    o->napx_sum = acc[ACC_NS];
  }
  if (want & TDTK_WANT_LUM) {
    for (int k = 0; k < 15; k++) o->lum[k] = acc[ACC_L + k];
    o->lum_udot = acc[ACC_LU];
  }
  if (want & TDTK_WANT_MOM2) {
    // second moments about the respective centroids
    const double* mm = acc + ACC_MM;
    const double* dd = acc + ACC_DD;
    int q = 0;
    for (int a = 0; a < 3; a++)
      for (int b = a; b < 3; b++, q++) {
        o->mom_mm[q] = mm[q] - Sm[a] * Sm[b] / n;
        o->mom_dd[q] = dd[q] - Sd[a] * Sd[b] / n;
      }
  }
  if (want & TDTK_WANT_GAPX) {
    // a = p1 - cm, b = p2 - cm (BOTH about centroid_m, gapx6D.cc:185-191); w = cm - shift = Sm/n
    double MM[3][3], DD[3][3], Saa[3][3], Sbb[3][3], Sab[3][3], Sb[3];
    const double* mm = acc + ACC_MM;
    const double* dd = acc + ACC_DD;
    MM[0][0] = mm[0]; MM[0][1] = MM[1][0] = mm[1]; MM[0][2] = MM[2][0] = mm[2];
    MM[1][1] = mm[3]; MM[1][2] = MM[2][1] = mm[4]; MM[2][2] = mm[5];
    DD[0][0] = dd[0]; DD[0][1] = DD[1][0] = dd[1]; DD[0][2] = DD[2][0] = dd[2];
    DD[1][1] = dd[3]; DD[1][2] = DD[2][1] = dd[4]; DD[2][2] = dd[5];
    for (int i = 0; i < 3; i++) {
      Sb[i] = Sd[i] - Sm[i];
      for (int j = 0; j < 3; j++) {
        Saa[i][j] = MM[i][j] - n * wm[i] * wm[j];
        Sbb[i][j] = DD[i][j] - wm[i] * Sd[j] - wm[j] * Sd[i] + n * wm[i] * wm[j];
        Sab[i][j] = acc[ACC_P + i * 3 + j] - wm[i] * Sd[j];
      }
    }
    auto sym = [](const double S[3][3], double* o9) {
      o9[0] = S[1][1] + S[2][2]; o9[1] = -S[0][1]; o9[2] = -S[0][2];
      o9[3] = -S[0][1]; o9[4] = S[0][0] + S[2][2]; o9[5] = -S[1][2];
      o9[6] = -S[0][2]; o9[7] = -S[1][2]; o9[8] = S[0][0] + S[1][1];
    };
    sym(Saa, o->gapx_MkMkt);
    sym(Sbb, o->gapx_DkDkt);
    // sum(p1 - cm) is zero by construction; the literal "+ p1y + p2y" terms leave sum(p2 - cm)
    const double d11 = Sab[1][1] + Sb[2], d22 = Sab[0][0] + Sb[2], d33 = Sab[0][0] + Sb[1];
    double* A = o->gapx_MkDkt;
    A[0] = d11; A[1] = -Sab[1][0]; A[2] = -Sab[2][0];
    A[3] = -Sab[1][0]; A[4] = d22; A[5] = -Sab[2][1];
    A[6] = -Sab[2][0]; A[7] = -Sab[2][1]; A[8] = d33;
    double* Bm = o->gapx_DkMkt;
    Bm[0] = d11; Bm[1] = -Sab[0][1]; Bm[2] = -Sab[0][2];
    Bm[3] = -Sab[0][1]; Bm[4] = d22; Bm[5] = -Sab[1][2];
    Bm[6] = -Sab[0][2]; Bm[7] = -Sab[1][2]; Bm[8] = d33;
    o->gapx_Ak2[0] = Sab[2][1] - Sab[1][2];
    o->gapx_Ak2[1] = Sab[0][2] - Sab[2][0];
    o->gapx_Ak2[2] = Sab[1][0] - Sab[0][1];
    for (int k = 0; k < 3; k++) o->gapx_Ak1[k] = -o->gapx_Ak2[k];
  }
}

// The pair sums of a pass land in pinned host memory, one 8-byte store per sum (k_final).  Waiting for them with
// hipStreamSynchronize costs ~6 us more per round trip on this box than watching the words themselves
// (tools/micro/sync_cost.hip: 12.7 against 6.3 us for an empty kernel), which is a sixth of a small scan's ICP iteration:
// the host arms every word with a NaN no sum can produce, launches, and reads until none is left.  The stream is asked
// now and then, so a failed launch ends the wait with its error and a finished stream ends it whatever the words say.
// TDTK_POLL_SUMS=0: hipStreamSynchronize.
static bool poll_sums()
{
  static const bool on = [] { const char* e = getenv("TDTK_POLL_SUMS"); return !(e && e[0] == '0'); }();
  return on;
}
static void arm_sums(double* h_pin)
{
  volatile uint64_t* w = reinterpret_cast<volatile uint64_t*>(h_pin);
  for (int k = 0; k < ACC_TOTAL; k++) w[k] = SUMS_ARMED;
}
// The wait is adaptive: the words are polled with a pause instruction between looks for TDTK_SPIN_US microseconds (default
// 30: an iteration over a small scan, 25-40 us, ends inside the window and keeps the 4 us it gains over
// hipStreamSynchronize); after that every look is followed by sched_yield(), so the 200 us kernel of a 1M-point
// iteration does not hold a core against the other threads of an OpenMP host (a yield with nobody waiting returns at
// once and costs the wait nothing).  The stream is asked now and then in both phases: a failed launch ends the wait
// with its error, a finished stream ends it whatever the words say.
static hipError_t await_sums(const double* h_pin, hipStream_t s)
{
  static const double spin_us = [] { const char* e = getenv("TDTK_SPIN_US"); const double v = e ? atof(e) : 30.0; return v < 0.0 ? 0.0 : v; }();
  const volatile uint64_t* w = reinterpret_cast<const volatile uint64_t*>(h_pin);
  const auto t0 = std::chrono::steady_clock::now();
  bool yielding = spin_us == 0.0;
  for (uint32_t spins = 1;; spins++) {
    bool all = true;
    for (int k = ACC_TOTAL - 1; k >= 0 && all; k--) all = w[k] != SUMS_ARMED;
    if (all) { std::atomic_thread_fence(std::memory_order_acquire); return hipSuccess; }
    if (yielding) {
      sched_yield();
      if ((spins & 0x3Fu) != 0) continue;
    } else {
      __builtin_ia32_pause();
      if ((spins & 0x3Fu) == 0 &&
          std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > spin_us) yielding = true;
      if ((spins & 0x3FFu) != 0) continue;
    }
    const hipError_t q = hipStreamQuery(s);
    if (q == hipSuccess) return hipSuccess;
    if (q != hipErrorNotReady) return q;
  }
}

// search + accumulate over a resident scan.  acc_out (host, ACC_TOTAL) receives raw columns.
// SearchArgs::tie (kernels.hip, "the quick check deferred"): the reference's quick check computes a = max_i(fabs(q_i - c_i) - h_i)
// with c = 0.5 * (min + max), h = 0.5 * (max - min) of the node's points; for a point p of the node and a query within the
// search radius R of it, a <= |q - p|_inf + E with E <= 8 * 2^-53 * (|min| + |max| + |q|) <= 2^-50 * (3 absmax + R), so a node
// the check cuts off (a * a >= closest_d2) holds only points with d2 >= closest_d2 - (2 E R + E^2).  Four times that, for the
// roundings of the comparison itself and of this expression; TDTK_DEFER_CHECK=0: every visit makes the check.
double search_margin(const tdtk_tree* t, double maxd2)
{
  if (!(maxd2 > 0.0) || !std::isfinite(maxd2)) return 0.0;
  const double R = std::sqrt(maxd2), E = std::ldexp(3.0 * (double)t->dev.absmax + R, -50);
  const double m = 4.0 * (2.0 * E * R + E * E);
  return (std::isfinite(m) && m < 1e-3 * maxd2) ? m : 0.0;
}
// The margin always widens a warm radius (SearchArgs::margin); whether the walk also DEFERS the quick check (SearchArgs::tie > 0)
// is a performance policy of its own:
static double search_tie(const tdtk_tree* t, double maxd2)
{
  static const bool off = [] { const char* e = getenv("TDTK_DEFER_CHECK"); return e && e[0] == '0'; }();
  if (off || !t->d_split) return 0.0;
  // Only for trees that live in the caches (the Infinity Cache is 256 MB): a walk without the quick check visits a sixth more
  // buckets, and once a bucket is a trip to HBM that costs more than the node loads it saves.  ICP iteration, k_search with
  // every check / with the check deferred: 1M-point tree (57 MB) 0.1665 / 0.1570 ms, 2M (115 MB) 0.357 / 0.334, 4M (230 MB)
  // 0.706 / 0.656, 10M-point city (0.65 GB) 1.28 / 1.37 (tools/r5_nobox_ab.sh, r5_defer_sizes.sh, r5_c5_waves.sh)
  static const size_t max_mb = [] { const char* e = lab_env("TDTK_DEFER_MAX_MB"); return e ? (size_t)atol(e) : (size_t)256; }();
  if (t->info.device_bytes > (max_mb << 20)) return 0.0;
  return search_margin(t, maxd2);
}

// The margin of a walk that leaves a certificate: m = clamp(kappa * move, lo * d, hi * d) (SearchArgs::cert_*; DESIGN section 4
// has the table the values were chosen from).  Any m >= 0 is exact; TDTK_CERT_KAPPA / _LO / _HI, read once per process, exist
// for repeating that table.
static void cert_policy(float* kappa, float* lo, float* hi)
{
  struct Policy { float kappa, lo, hi; };
  static const Policy pol = [] {
    auto env = [](const char* name, float dflt) {
      const char* e = getenv(name);
      if (!e || !e[0]) return dflt;
      const float v = (float)atof(e);
      return (v >= 0.f && v <= 1024.f) ? v : dflt;
    };
    return Policy{env("TDTK_CERT_KAPPA", 4.0f), env("TDTK_CERT_LO", 1.0f / 64.0f), env("TDTK_CERT_HI", 0.25f)};
  }();
  *kappa = pol.kappa; *lo = pol.lo; *hi = pol.hi;
}

// the accumulation point of a pass: the tree's box centre moved by A
void pass_shift(const tdtk_tree* t, const double* A16, double out[3])
{
  for (int k = 0; k < 3; k++) out[k] = t->centre[0] * A16[k] + t->centre[1] * A16[4 + k] + t->centre[2] * A16[8 + k] + A16[12 + k];
}

int scan_pass(Ctx* c, const tdtk_tree* model, const double* A16, tdtk_scan* data, int pmode, double maxd2,
              unsigned want, const double* lum_D, const double* pending, bool do_search, double* acc_out,
              double shift_out[3], bool warm, const unsigned char* skip, bool cert_ok)
{
  hipStream_t s = c->stream;
  const size_t N = data->N;
  int rc = c->ws[WS_KPOS].ensure(N * sizeof(int));
  if (rc) return rc;
  if ((rc = scan_settle(c, data))) return rc;
  Mat4 A, inv;
  std::memcpy(A.m, A16, sizeof A.m);
  m4inv(A16, inv.m);  // searchTree.cc:110
  // sums are taken about the model box centre mapped to the world: keeps the raw second
  // moments small so the centred covariance survives the subtraction in fp64
  double sh[3];
  pass_shift(model, A16, sh);
  for (int k = 0; k < 3; k++) shift_out[k] = sh[k];
  // the base block (n, sum, centroids, Si) of a closest-point pass comes out of the search kernel itself when the
  // batch is large enough for the persistent-lane kernel (retire-time accumulation, kernels.hip)
  const int fmode = (do_search && pmode == 0 && (want & ~TDTK_WANT_BASE) == 0 && !lum_D) ? fuse_mode(N) : 0;
  const bool fused = fmode != 0 && !(fmode == 4 && c->counting);   // (the instrumented small-batch kernels have no epilogue)
  if (do_search) {
    SearchArgs sa{};
    sa.x = data->x; sa.y = data->y; sa.z = data->z;
    sa.nx = data->nx; sa.ny = data->ny; sa.nz = data->nz;
    sa.n = N;
    sa.has_pending = pending ? 1 : 0;
    if (pending) std::memcpy(sa.pending.m, pending, sizeof sa.pending.m);
    sa.inv = inv; sa.has_inv = 1;
    sa.maxd2 = maxd2;
    sa.kpos = c->ws[WS_KPOS].as<int>();
    sa.skip = skip;
    sa.warm = (warm && pmode != 1 && !c->count_cold) ? 1 : 0;   // WS_KPOS still holds this scan's hits in this tree from the last pass
    sa.margin = sa.warm ? search_margin(model, maxd2) : 0.0;
    sa.tie = sa.warm ? search_tie(model, maxd2) : 0.0;
    {
      // ... and WS_COST how many buckets each of its queries visited then: the persistent-lane kernel hands a wave's slab
      // out with the expensive queries first (TDTK_COST_ORDER=0: in slab order)
      const char* co = lab_env("TDTK_COST_ORDER");
      if (pmode != 1 && !(co && co[0] == '0') && search_fuse_kind(N) == 1) {
        if ((rc = c->ws[WS_COST].ensure(N))) return rc;
        sa.cost = c->ws[WS_COST].as<unsigned char>();
        sa.use_cost = sa.warm;
      }
    }
    sa.d2 = nullptr;
#ifdef TDTK_LAB
    // lab (a measured negative, NEGATIVES.md): slabs of equal cost, cut by the previous pass of this loop behind its k_final;
    // TDTK_BALANCE=1 turns it on
    if (sa.use_cost && c->next_bounds && c->next_bounds_n == N) sa.bounds = c->next_bounds;
    c->next_bounds = nullptr;
    const bool cut_next = sa.cost != nullptr && search_fuse_after_last_pays(N) && [] { const char* e = lab_env("TDTK_BALANCE"); return e && e[0] == '1'; }();
    auto cut_slabs = [&]() -> int {     // enqueued behind the pass's last kernel: runs while the host solves for the pose
      if (!cut_next) return TDTK_OK;
      const void* before = c->ws[WS_BOUNDS].p;
      int r2 = c->ws[WS_BOUNDS].ensure(slab_bounds_bytes(N));
      if (r2) return r2;
      if (c->ws[WS_BOUNDS].p != before) HIPCHK(hipMemsetAsync(c->ws[WS_BOUNDS].p, 0, 256, s));
      const uint32_t* b = nullptr;
      HIPCHK(launch_slab_bounds(sa.cost, N, c->ws[WS_BOUNDS].p, &b, s));
      c->next_bounds = b; c->next_bounds_n = N;
      return TDTK_OK;
    };
#else
    auto cut_slabs = []() -> int { return TDTK_OK; };
#endif
    uint32_t rows = 0;
    if (fused) {
      rows = search_fused_rows(N);
      if ((rc = c->ws[WS_PART].ensure((size_t)rows * ACC_TOTAL * sizeof(double)))) return rc;
      sa.fuse = fmode; sa.A = A;
      for (int k = 0; k < 3; k++) sa.shift[k] = sh[k];
      sa.partials = c->ws[WS_PART].as<double>();
    }
    // Certificates (kernels.hip, "a certificate per query"): only between consecutive passes of one tdtk_icp_match loop (cert_ok:
    // the loop says so; TDTK_CERT_SKIP=0: never) that both run the instantiation that keeps them.  The first such pass ignores what
    // the array holds and writes it, the following ones use it; any other pass of this context ends the chain.
    bool certs = false;
    if (cert_ok && fused && pmode == 0 && !skip) {
      sa.T = model->dev;
      certs = search_cert_capable(sa);
    }
    if (certs) {
      if ((rc = c->ws[WS_CERT].ensure(N * sizeof(float)))) return rc;
      sa.cert = c->ws[WS_CERT].as<float>();
      sa.cert_use = c->cert_live ? 1 : 0;
      cert_policy(&sa.cert_kappa, &sa.cert_lo, &sa.cert_hi);
    }
    c->cert_live = certs;
    rc = run_search(c, model, sa, pmode == 1 ? 1 : 0, false, s, true);
    if (rc) return rc;
    if (fused) {
      const bool tm = kernel_timing();
      if (tm) HIPCHK(hipEventRecord(c->e2, s));
      const bool poll = !tm && poll_sums();
      if (poll) arm_sums(c->h_pin);
      HIPCHK(launch_final(sa.partials, rows, c->h_pin, s, (fmode == 3 || fmode == 4) ? (int)ACC_DD : (int)ACC_TOTAL));   // base block only
      if (tm) { HIPCHK(hipEventRecord(c->e3, s)); c->ev2_pending = true; }
      if ((rc = cut_slabs())) return rc;
      if (poll) HIPCHK(await_sums(c->h_pin, s));
      else HIPCHK(hipStreamSynchronize(s));
      std::memcpy(acc_out, c->h_pin, ACC_TOTAL * sizeof(double));
      return TDTK_OK;
    }
    if ((rc = cut_slabs())) return rc;      // (before k_accum: the cut needs the cost bytes only)
  }
  AccumArgs aa{};
  aa.T = model->dev;
  aa.x = data->x; aa.y = data->y; aa.z = data->z;
  aa.nx = data->nx; aa.ny = data->ny; aa.nz = data->nz;
  aa.kpos = c->ws[WS_KPOS].as<int>();
  aa.n = N;
  aa.A = A; aa.inv = inv;
  for (int k = 0; k < 3; k++) aa.shift[k] = sh[k];
  aa.has_D = lum_D ? 1 : 0;
  if (lum_D) std::memcpy(aa.D, lum_D, sizeof aa.D);
  const uint32_t grid = accum_grid(N);
  rc = c->ws[WS_PART].ensure((size_t)grid * ACC_TOTAL * sizeof(double));
  if (rc) return rc;
  aa.partials = c->ws[WS_PART].as<double>();
  // k_final stores the 74 sums straight into pinned host memory (device-visible): no copy-engine hop
  // between the last kernel and the host solve, which matters when an iteration is ~100 us
  const bool tm = kernel_timing();
  if (tm) HIPCHK(hipEventRecord(c->e2, s));
  const bool poll = !tm && poll_sums();
  if (poll) arm_sums(c->h_pin);
  HIPCHK(launch_accum(aa, grid, want, pmode, c->h_pin, s));
  if (tm) { HIPCHK(hipEventRecord(c->e3, s)); c->ev2_pending = true; }
  if (poll) HIPCHK(await_sums(c->h_pin, s));
  else HIPCHK(hipStreamSynchronize(s));
  std::memcpy(acc_out, c->h_pin, ACC_TOTAL * sizeof(double));
  return TDTK_OK;
}

int scan_idx_to_host(Ctx* c, const tdtk_tree* model, tdtk_scan* data, int32_t* idx_out)
{
  const size_t N = data->N;
  int rc = c->ws[WS_IDX].ensure(N * sizeof(int32_t));
  if (rc) return rc;
  HIPCHK(launch_scatter_idx(c->ws[WS_KPOS].as<int>(), nullptr, data->d_order, model->dev.pts, N,
                            c->ws[WS_IDX].as<int32_t>(), nullptr, c->stream));
  HIPCHK(hipMemcpyAsync(idx_out, c->ws[WS_IDX].p, N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TDTK_OK;
}

}  // namespace tdtk

// an unsorted batch binned over the tree's root box, 32 cells per axis: the queries (and their directions) sorted into
// WS_QX.. (WS_DX..), their order into WS_ORDER -- the caller has sized the workspaces
static BinArgs bin_args(Ctx* c, const tdtk_tree* t, const double* d_q, const double* d_dir, size_t K)
{
  BinArgs b{};
  b.q = d_q; b.dir = d_dir; b.n = K;
  for (int a = 0; a < 3; a++) {
    b.lo[a] = t->bbmin[a];
    const double ext = t->bbmax[a] - t->bbmin[a];
    b.scale[a] = (ext > 0) ? 32.0 / ext : 0.0;
  }
  b.hist = c->ws[WS_HIST].as<uint32_t>();
  b.cell = c->ws[WS_CELL].as<uint32_t>();
  b.sx = c->ws[WS_QX].as<double>(); b.sy = c->ws[WS_QY].as<double>(); b.sz = c->ws[WS_QZ].as<double>();
  if (d_dir) { b.sdx = c->ws[WS_DX].as<double>(); b.sdy = c->ws[WS_DY].as<double>(); b.sdz = c->ws[WS_DZ].as<double>(); }
  b.order = c->ws[WS_ORDER].as<int32_t>();
  return b;
}

extern "C" {

// ---- find closest ----------------------------------------------------------------------
int tdtk_find_closest_dev(const tdtk_tree* t, const double* d_q, size_t K, double maxdist2,
                          int32_t* d_idx, double* d_d2, int presorted, void* stream)
{
  if (!t || (!d_q && K)) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(t->device, &c);
  if (rc) return rc;
  if (K == 0) return TDTK_OK;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  int ids[] = {WS_QX, WS_QY, WS_QZ};
  for (int id : ids)
    if ((rc = c->ws[id].ensure(K * sizeof(double)))) return rc;
  if ((rc = c->ws[WS_KPOS].ensure(K * sizeof(int)))) return rc;
  if ((rc = c->ws[WS_D2].ensure(K * sizeof(double)))) return rc;
  const int32_t* order = nullptr;
  if (!presorted) {
    if ((rc = c->ws[WS_ORDER].ensure(K * sizeof(int32_t)))) return rc;
    if ((rc = c->ws[WS_CELL].ensure(K * sizeof(uint32_t)))) return rc;
    if ((rc = c->ws[WS_HIST].ensure(32768 * sizeof(uint32_t)))) return rc;
    const BinArgs b = bin_args(c, t, d_q, nullptr, K);
    HIPCHK(launch_bin(b, s));
    order = b.order;
  } else {
    HIPCHK(launch_split_soa(d_q, K, c->ws[WS_QX].as<double>(), c->ws[WS_QY].as<double>(),
                            c->ws[WS_QZ].as<double>(), s));
  }
  SearchArgs sa{};
  sa.x = c->ws[WS_QX].as<double>(); sa.y = c->ws[WS_QY].as<double>(); sa.z = c->ws[WS_QZ].as<double>();
  sa.n = K; sa.maxd2 = maxdist2;
  sa.kpos = c->ws[WS_KPOS].as<int>();
  sa.d2 = c->ws[WS_D2].as<double>();
  rc = run_search(c, t, sa, 0, false, s, true);
  if (rc) return rc;
  HIPCHK(launch_scatter_idx(sa.kpos, sa.d2, order, t->dev.pts, K, d_idx, d_d2, s));
  if (!stream) HIPCHK(hipStreamSynchronize(s));
  else {
    // the kernels queued on the caller's stream use this thread's workspaces: whatever this thread's own stream
    // does next (any later tdtk call) waits for them, so the buffers are never overwritten under a running kernel
    HIPCHK(hipEventRecord(c->e_user, s));
    HIPCHK(hipStreamWaitEvent(c->stream, c->e_user, 0));
  }
  return TDTK_OK;
}

int tdtk_find_closest(const tdtk_tree* t, const double* q, size_t K, double maxdist2, int32_t* idx,
                      double* d2)
{
  if (!t || (!q && K) || (!idx && K)) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(t->device, &c);
  if (rc) return rc;
  if (K == 0) return TDTK_OK;
  if ((rc = c->ws[WS_TMPA].ensure(3 * K * sizeof(double)))) return rc;
  if ((rc = c->ws[WS_IDX].ensure(K * sizeof(int32_t)))) return rc;
  if ((rc = c->ws[WS_TMPB].ensure(K * sizeof(double)))) return rc;
  HIPCHK(hipMemcpyAsync(c->ws[WS_TMPA].p, q, 3 * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
  rc = tdtk_find_closest_dev(t, c->ws[WS_TMPA].as<double>(), K, maxdist2, c->ws[WS_IDX].as<int32_t>(),
                             c->ws[WS_TMPB].as<double>(), 0, c->stream);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(idx, c->ws[WS_IDX].p, K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (d2) HIPCHK(hipMemcpyAsync(d2, c->ws[WS_TMPB].p, K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TDTK_OK;
}

int tdtk_find_closest_along_dir(const tdtk_tree* t, const double* q, const double* dir, size_t K,
                                double maxdist2, int32_t* idx, double* d2)
{
  if (!t || ((!q || !dir || !idx) && K)) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(t->device, &c);
  if (rc) return rc;
  if (K == 0) return TDTK_OK;
  hipStream_t s = c->stream;
  int dbl[] = {WS_QX, WS_QY, WS_QZ, WS_DX, WS_DY, WS_DZ, WS_D2, WS_TMPB};
  for (int id : dbl)
    if ((rc = c->ws[id].ensure(K * sizeof(double)))) return rc;
  if ((rc = c->ws[WS_TMPA].ensure(6 * K * sizeof(double)))) return rc;
  if ((rc = c->ws[WS_KPOS].ensure(K * sizeof(int)))) return rc;
  if ((rc = c->ws[WS_IDX].ensure(K * sizeof(int32_t)))) return rc;
  if ((rc = c->ws[WS_ORDER].ensure(K * sizeof(int32_t)))) return rc;
  if ((rc = c->ws[WS_CELL].ensure(K * sizeof(uint32_t)))) return rc;
  if ((rc = c->ws[WS_HIST].ensure(32768 * sizeof(uint32_t)))) return rc;
  double* dq = c->ws[WS_TMPA].as<double>();
  double* dd = dq + 3 * K;
  HIPCHK(hipMemcpyAsync(dq, q, 3 * K * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dd, dir, 3 * K * sizeof(double), hipMemcpyHostToDevice, s));
  const BinArgs b = bin_args(c, t, dq, dd, K);
  HIPCHK(launch_bin(b, s));
  SearchArgs sa{};
  sa.x = b.sx; sa.y = b.sy; sa.z = b.sz;
  sa.nx = b.sdx; sa.ny = b.sdy; sa.nz = b.sdz;
  sa.n = K; sa.maxd2 = maxdist2;
  sa.kpos = c->ws[WS_KPOS].as<int>();
  sa.d2 = c->ws[WS_D2].as<double>();
  rc = run_search(c, t, sa, 2, false, s, true);
  if (rc) return rc;
  HIPCHK(launch_scatter_idx(sa.kpos, sa.d2, b.order, t->dev.pts, K, c->ws[WS_IDX].as<int32_t>(),
                            c->ws[WS_TMPB].as<double>(), s));
  HIPCHK(hipMemcpyAsync(idx, c->ws[WS_IDX].p, K * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (d2) HIPCHK(hipMemcpyAsync(d2, c->ws[WS_TMPB].p, K * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return TDTK_OK;
}

int tdtk_count_visits(const tdtk_tree* t, const double* q, size_t K, double maxdist2, uint64_t counters[3])
{
  if (!t || !q || !counters) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(t->device, &c);
  if (rc) return rc;
  hipStream_t s = c->stream;
  int ids[] = {WS_QX, WS_QY, WS_QZ};
  for (int id : ids)
    if ((rc = c->ws[id].ensure(K * sizeof(double)))) return rc;
  if ((rc = c->ws[WS_TMPA].ensure(3 * K * sizeof(double)))) return rc;
  if ((rc = c->ws[WS_KPOS].ensure(K * sizeof(int)))) return rc;
  if ((rc = c->ws[WS_CNT].ensure(3 * sizeof(unsigned long long)))) return rc;
  HIPCHK(hipMemcpyAsync(c->ws[WS_TMPA].p, q, 3 * K * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(c->ws[WS_CNT].p, 0, 3 * sizeof(unsigned long long), s));
  HIPCHK(launch_split_soa(c->ws[WS_TMPA].as<double>(), K, c->ws[WS_QX].as<double>(),
                          c->ws[WS_QY].as<double>(), c->ws[WS_QZ].as<double>(), s));
  SearchArgs sa{};
  sa.x = c->ws[WS_QX].as<double>(); sa.y = c->ws[WS_QY].as<double>(); sa.z = c->ws[WS_QZ].as<double>();
  sa.n = K; sa.maxd2 = maxdist2;
  sa.kpos = c->ws[WS_KPOS].as<int>();
  sa.counters = c->ws[WS_CNT].as<unsigned long long>();
  rc = run_search(c, t, sa, 0, true, s, false);
  if (rc) return rc;
  unsigned long long h[3];
  HIPCHK(hipMemcpyAsync(h, c->ws[WS_CNT].p, sizeof h, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (int k = 0; k < 3; k++) counters[k] = h[k];
  return TDTK_OK;
}

// this thread's context on the current device (the timing read-outs name no device and touch no scan)
static int current_ctx(Ctx** c)
{
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { set_error("no device"); return TDTK_EDEVICE; }
  return get_ctx(dev, c, false);
}

int tdtk_last_kernel_ms(double* nn_ms)
{
  Ctx* c;
  int rc = current_ctx(&c);
  if (rc) return rc;
  return collect_ms(c, nn_ms);
}

int tdtk_kernel_timing(int on)
{
  const int was = kernel_timing() ? 1 : 0;
  g_kernel_timing.store(on ? 1 : 0, std::memory_order_relaxed);
  return was;
}

int tdtk_last_timings(double out[4])
{
  if (!out) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = current_ctx(&c);
  if (rc) return rc;
  rc = collect_ms(c, &out[0], &out[1]);
  out[2] = c->last_normals_ms;
  out[3] = c->last_build_ms;
  return rc;
}

// every FindClosest pass this thread runs on `device` from now on uses the instrumented instantiation of the
// kernel it would have used (same traversal, same warm radius, same results) and adds to the counters; on == 2: the
// searches also start cold (no warm start, no deferred quick check): what the counters then hold is the walk of the
// reference's _FindClosest (kdTreeImpl.h:345-383) -- SURVEY 8(d)'s n_int / n_pts -- on the same queries, same results
int tdtk_visit_counting(int device, int on)
{
  Ctx* c;
  int rc = get_ctx(device, &c);
  if (rc) return rc;
  if (on) {
    if ((rc = c->d_counters.ensure(16 * sizeof(unsigned long long)))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemset(c->d_counters.p, 0, 16 * sizeof(unsigned long long)));
    c->counted_queries = 0;
    c->counted_ann_queries = 0;
  }
  c->counting = on != 0;
  c->count_cold = on == 2;
  return TDTK_OK;
}

int tdtk_visit_counters(int device, uint64_t out[8])
{
  if (!out) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(device, &c);
  if (rc) return rc;
  for (int k = 0; k < 8; k++) out[k] = 0;
  out[3] = c->counted_queries;
  out[6] = c->counted_ann_queries;
  if (!c->d_counters.p) return TDTK_OK;
  HIPCHK(hipDeviceSynchronize());   // link passes run on auxiliary streams
  unsigned long long h[8];
  HIPCHK(hipMemcpy(h, c->d_counters.p, sizeof h, hipMemcpyDeviceToHost));
  for (int k = 0; k < 3; k++) out[k] = h[k];
  out[4] = h[4]; out[5] = h[5];
  out[7] = h[7];
  return TDTK_OK;
}

// the instrumented persistent-lane launches since tdtk_visit_counting(device, on): queries answered by their certificate with
// the hit kept (out[0]) and without a hit (out[1]), queries handed to a lane (out[2]), second searches behind a slab (out[3])
int tdtk_skip_counters(int device, uint64_t out[4])
{
  if (!out) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(device, &c);
  if (rc) return rc;
  for (int k = 0; k < 4; k++) out[k] = 0;
  if (!c->d_counters.p) return TDTK_OK;
  HIPCHK(hipDeviceSynchronize());
  unsigned long long h[16];
  HIPCHK(hipMemcpy(h, c->d_counters.p, sizeof h, hipMemcpyDeviceToHost));
  out[0] = h[10]; out[1] = h[11]; out[2] = h[12]; out[3] = h[7];
  return TDTK_OK;
}

#ifdef TDTK_LAB
// lab: trips of the waves of the instrumented persistent-lane launches since tdtk_visit_counting(device, 1) through the node
// walk (out[0]) and the bucket scan (out[1]): with the visit counters, lane-visits / (64 x trips) = how full a phase's trips are
extern "C" int tdtk_lab_trip_counters(int device, uint64_t out[2])
{
  if (!out) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(device, &c);
  if (rc) return rc;
  out[0] = out[1] = 0;
  if (!c->d_counters.p) return TDTK_OK;
  HIPCHK(hipDeviceSynchronize());
  unsigned long long h[2];
  HIPCHK(hipMemcpy(h, c->d_counters.as<unsigned long long>() + 8, sizeof h, hipMemcpyDeviceToHost));
  out[0] = h[0]; out[1] = h[1];
  return TDTK_OK;
}
#endif

// measured roofline denominators: kind 0 = HBM stream copy (16 B per lane, `bytes` read + `bytes`
// written per pass, the buffers far beyond the 256 MB Infinity Cache when bytes >= 1 GB); kind 1 = repeated reads of
// a buffer that fits the L2s (bytes <= 16 MB: every workgroup sweeps its own XCD-local slice); GB/s of the best pass.
int tdtk_measure_bandwidth(int device, int kind, size_t bytes, int reps, double* gbs)
{
  if (!gbs || bytes < 4096 || reps < 1 || kind < 0 || kind > 1) { set_error("bad argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(device, &c);
  if (rc) return rc;
  bytes &= ~(size_t)4095;
  DevBuf a, b;
  if ((rc = a.ensure(bytes))) return rc;
  if (kind == 0 && (rc = b.ensure(bytes))) return rc;
  HIPCHK(hipMemsetAsync(a.p, 1, bytes, c->stream));
  double best = 0.0;
  const int variants[3] = {0, 2, 3};          // stream copy: plain, non-temporal, larger grid -- the best one counts
  for (int v = 0; v < (kind == 0 ? 3 : 1); v++)
    for (int r = 0; r < reps + 1; r++) {
      HIPCHK(hipEventRecord(c->e0, c->stream));
      double moved = 0.0;
      HIPCHK(launch_bandwidth(kind == 0 ? variants[v] : kind, a.p, b.p, bytes, &moved, c->stream));
      HIPCHK(hipEventRecord(c->e1, c->stream));
      HIPCHK(hipEventSynchronize(c->e1));
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, c->e0, c->e1));
      if (r > 0 && ms > 0) best = std::max(best, moved / (ms * 1e-3) / 1e9);
    }
  *gbs = best;
  return TDTK_OK;
}

}  // extern "C"
