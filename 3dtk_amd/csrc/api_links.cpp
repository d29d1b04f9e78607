// Whole-scan passes over the links of a graph: one lum6DEuler link, the policies of a batch of links, the batched launch
// and the lanes, and the entry points that turn the passes' sums into pair sums and lum6DEuler blocks.
#include "api_internal.h"

using namespace tdtk;

extern "C" {

// ---- lum6DEuler::covarianceEuler -----------------------------------------------------------
// the normal system of one link: MM (6 x 6) from the pair count m and the nine sums L[0..8], and D = MM^-1 MZ, MZ = L[9..14]
static int lum_normal_system(uint64_t m, const double* L, double MM[36], double D[6])
{
  const double* MZ = L + 9;
  const double sx = L[0], sy = L[1], sz = L[2], xpy = L[3], xpz = L[4], ypz = L[5], xy = L[6], xz = L[7], yz = L[8];
  std::memset(MM, 0, 36 * sizeof(double));
  auto M = [&](int r, int col) -> double& { return MM[(r - 1) * 6 + (col - 1)]; };  // 1-based like newmat
  M(1, 1) = M(2, 2) = M(3, 3) = (double)m;
  M(4, 4) = ypz; M(5, 5) = xpy; M(6, 6) = xpz;
  M(1, 5) = M(5, 1) = -sy; M(1, 6) = M(6, 1) = sz;
  M(2, 4) = M(4, 2) = -sz; M(2, 5) = M(5, 2) = sx;
  M(3, 4) = M(4, 3) = sy;  M(3, 6) = M(6, 3) = -sx;
  M(4, 5) = M(5, 4) = -xz; M(4, 6) = M(6, 4) = -xy; M(5, 6) = M(6, 5) = -yz;
  double MMi[36];
  if (!invert_dense(6, MM, MMi)) { set_error("singular link matrix"); return TDTK_ESOLVE; }
  for (int r = 0; r < 6; r++) {
    double v = 0;
    for (int k = 0; k < 6; k++) v += MMi[r * 6 + k] * MZ[k];
    D[r] = v;
  }
  return TDTK_OK;
}

int tdtk_lum_link(const tdtk_tree* first, const double first_dalignxf[16], tdtk_scan* second, double maxd2,
                  double C[36], double CD[6], uint64_t* m_out, double* ss_out)
{
  if (!first || !first_dalignxf || !second || !C || !CD) { set_error("NULL argument"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(first->device, &c);
  if (rc) return rc;
  std::memset(C, 0, 36 * sizeof(double));
  std::memset(CD, 0, 6 * sizeof(double));
  if (m_out) *m_out = 0;
  if (ss_out) *ss_out = 0;
  if (second->N == 0) return TDTK_OK;
  double acc[ACC_TOTAL], shift[3];
  rc = scan_pass(c, first, first_dalignxf, second, 0, maxd2, TDTK_WANT_LUM, nullptr, nullptr, true, acc, shift);
  if (rc) return rc;
  collect_ms(c, nullptr);
  const uint64_t m = (uint64_t)(acc[ACC_N] + 0.5);
  if (m_out) *m_out = m;
  if (m <= 2) return TDTK_OK;  // "This case should not occur": zeros (lum6Deuler.cc:234-249)
  const double* L = acc + ACC_L;
  const double* MZ = L + 9;
  double MM[36], D[6];
  if ((rc = lum_normal_system(m, L, MM, D))) return rc;
  // second pass over the same correspondences (kpos is still in the workspace)
  double acc2[ACC_TOTAL];
  rc = scan_pass(c, first, first_dalignxf, second, 0, maxd2, TDTK_WANT_LUM, D, nullptr, false, acc2, shift);
  if (rc) return rc;
  double ss = acc2[ACC_LSS] / (2.0 * (double)m - 3.0);
  if (ss_out) *ss_out = ss;
  if (ss < 0.0000000000001) return TDTK_OK;  // lum6Deuler.cc:215-226: zeros
  ss = 1.0 / ss;
  for (int k = 0; k < 36; k++) C[k] = MM[k] * ss;
  for (int k = 0; k < 6; k++) CD[k] = MZ[k] * ss;
  return TDTK_OK;
}

// ---- batched whole-scan passes over a list of links --------------------------------------------
// search + sums of every link, kernels enqueued back to back, one host sync.  Links over small scans are dealt to
// up to 8 auxiliary streams (each pass alone leaves most of the machine idle); big scans keep the one stream.
// acc: [nlinks][ACC_TOTAL] raw columns; shifts: [nlinks][3].
static bool fuse_lum_enabled()
{
  const char* e = lab_env("TDTK_FUSE_LUM");
  return e && e[0] == '1';
}

static int link_batch_max()
{
  const char* e = lab_env("TDTK_LINK_BATCH");   // 0 / 1: the lanes below
  int v = e ? atoi(e) : 128;   // (84 links of 1M points: one launch 11.20 ms per LUM round, 64 + 20: 11.22-11.27, 42 + 42: 11.22)
  if (v > 128) v = 128;
  return v;
}

// The 17 sums of a lum6DEuler link added up by the search waves themselves, each over its own slab after its last query
// (k_search_refill_multi<.., 5>): the pass over (x, y, z, hit, pts[hit]) that k_accum_multi makes disappears into the
// search launch -- 84 links of 1M points: search 8.9 -> 9.5 ms, pair sums 1.04 -> 0, LUM round 10.95 -> 10.55 ms.  The rows
// of partial sums are then the slabs, so every such launch uses one slab length and a lone link takes this path too: a
// link's sums do not depend on how many links (or ranks) share the work.  TDTK_LINK_FUSE=0: k_accum_multi.
static bool link_sums_in_search(const Ctx* c, unsigned want, size_t maxN)
{
  const char* e = lab_env("TDTK_LINK_FUSE");
  if (e && e[0] == '0') return false;
  // (experiments with the slab layout change the rows; TDTK_LINK_FUSE=2 keeps the sums inside for such sweeps)
  if ((lab_env("TDTK_REFILL_QPW") || lab_env("TDTK_LINK_PHASES")) && !(e && e[0] == '2')) return false;
  const int th = search_multi_thresh(maxN);
  return !c->counting && want == (TDTK_WANT_LUM | ACC_WANT_NO_CROSS) && search_multi_class(maxN) == 20 && (th == 16 || th == 32);
}

// All links of the call in launches of up to `gb` links each: ONE search launch, one pair-sum launch and one final
// reduction per group (k_search_refill_multi and friends: workgroups of link k+1 fill the tail of link k), everything on
// the context's stream -- what the lanes below get from three streams, without depending on how the runtime maps streams
// to hardware queues, and with a handful of launches instead of three per link.
static int links_device_pass_batched(Ctx* c, int nlinks, const tdtk_tree* const* first, const double* first_dalignxf,
                                     tdtk_scan* const* second, double maxd2, unsigned want, double* d_out,
                                     const std::vector<double>& shifts, int gb)
{
  hipStream_t s = c->stream;
  int rc;
  size_t maxN = 0;
  int max_need = 0;
  for (int i = 0; i < nlinks; i++) {
    maxN = std::max(maxN, second[i]->N);
    max_need = std::max(max_need, (int)first[i]->info.max_depth - 1 - search_lds_depth());
  }
  const int G = std::min(gb, nlinks);
  // A wave hands out each piece of its slab with the queries that were expensive in the previous pass of the same link
  // first, as the single pass does (k_search_refill, ORDER): 84 links of 1M points 9.18 -> 8.91 ms per LUM round.  The
  // order changes which lanes share a trip, never a result.  TDTK_LINK_ORDERED=0: in slab order.
  const bool ordered_env = [] { const char* e = lab_env("TDTK_LINK_ORDERED"); return !(e && e[0] == '0'); }();   // (per call: tests flip it)
  const bool ordered = ordered_env && !c->counting && search_multi_class(maxN) == 20;
  const bool fuse_links = link_sums_in_search(c, want, maxN);
  if (ordered) {
    while ((int)c->link_costs.size() < nlinks) c->link_costs.emplace_back(new LinkCost);
    for (int p = 0; p < nlinks; p++) {
      LinkCost* lc = c->link_costs[p].get();
      const void* before = lc->cost.p;
      if ((rc = lc->cost.ensure(maxN))) return rc;
      if (lc->cost.p != before) lc->tree = nullptr;
    }
  }
  while ((int)c->slots.size() < G) c->slots.emplace_back(new Lane);
  for (int g = 0; g < G; g++) {          // every buffer at its final size before anything is enqueued
    Lane* sl = c->slots[g].get();
    {
      const void* before = sl->kpos.p;
      if ((rc = sl->kpos.ensure(maxN * sizeof(int)))) return rc;
      if (sl->kpos.p != before) sl->k_tree = sl->k_scan = 0;
    }
    {
      size_t rows = accum_grid(maxN);
      if (fuse_links) {
        SearchArgs probe{};
        probe.n = maxN;
        rows = std::max<size_t>(rows, search_multi_prepare(probe, G, true));
      }
      if ((rc = sl->part.ensure(rows * ACC_TOTAL * sizeof(double)))) return rc;
    }
    if (max_need > 0) {
      // the stack overflow area of a batch: one column per lane of ITS grid (a tenth of what the stand-alone kernels'
      // common area needs, and there are up to 128 of these)
      SearchArgs probe{};
      probe.n = maxN;
      const size_t lanes = (size_t)std::max(search_multi_prepare(probe, 1, fuse_links), search_multi_prepare(probe, G, fuse_links)) * 256;   // the shortest slab any
                                                                                                        // group gets; 256: the widest workgroup
      if ((rc = sl->ovf_m2.ensure(lanes * max_need * sizeof(double)))) return rc;
      if ((rc = sl->ovf_ref.ensure(lanes * max_need * sizeof(uint32_t)))) return rc;
    }
  }
  const int ngroups = (nlinks + G - 1) / G;
  // Launch order: links that search the SAME tree next to each other (a chain link i -> i+1 and the loop closures out
  // of scan i), so that the tree one of them has pulled into the L2s / the Infinity Cache is still there for the next;
  // otherwise the caller's order.  The workgroups of a launch are dispatched in table order, so position p of the table
  // is what runs p-th; every link still writes its own row of d_out (TDTK_LINK_ORDER=0: the caller's order).
  std::vector<int> ord(nlinks);
  for (int i = 0; i < nlinks; i++) ord[i] = i;
  {
    static const bool keep = [] { const char* e = lab_env("TDTK_LINK_ORDER"); return e && e[0] == '0'; }();
    if (!keep) {
      std::map<const tdtk_tree*, int> seen;
      std::vector<int> key(nlinks);
      for (int i = 0; i < nlinks; i++) key[i] = seen.emplace(first[i], i).first->second;   // first link that uses this tree
      std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return key[a] < key[b]; });
    }
  }
  // Lazy scan moves (tdtk_scan::pending): the persistent-lane launch carries them out itself; the small-batch kernels do
  // not, their scans are moved first.  Everything that can fail is done before the first scan's state changes.
  const bool lazy = search_multi_class(maxN) == 20;
  const bool link_warm = [] { const char* e = lab_env("TDTK_LINK_WARM"); return !(e && e[0] == '0'); }();
  size_t nmat_max = 0;
  if (!lazy) {
    if ((rc = scans_settle(c, second, nlinks))) return rc;
  } else {
    {   // a chain longer than the launch applies itself (a scan no link of this rank has read for rounds): one pass now
      std::vector<const tdtk_scan*> longc;
      for (int i = 0; i < nlinks; i++)
        if (second[i]->pending.size() > (size_t)SEARCH_LAZY_MAX) longc.push_back(second[i]);
      if (!longc.empty() && (rc = scans_settle(c, longc.data(), (int)longc.size()))) return rc;
    }
    {   // a copy of its own for every reader of a moving scan but the first of its launch (which gets the spare arrays)
      std::map<const tdtk_scan*, int> first_in;      // scan -> the launch that moves it
      for (int p = 0; p < nlinks; p++) {
        const tdtk_scan* sc = second[ord[p]];
        if (sc->pending.empty()) continue;
        const int gi = p / G;
        const auto it = first_in.find(sc);
        if (it == first_in.end()) first_in[sc] = gi;
        else if (it->second == gi && (rc = c->slots[p - gi * G]->moved.ensure(3 * maxN * sizeof(double)))) return rc;
      }
    }
    for (int i = 0; i < nlinks; i++) {
      tdtk_scan* sc = second[i];
      if (sc->pending.empty()) continue;
      nmat_max += sc->pending.size();
      if ((rc = scan_ensure_spare(sc))) return rc;
    }
  }
  // one table for the whole call: per link its search and pair-sum arguments and final descriptor, per group the two
  // workgroup-offset lists, then the chains of queued moves
  const size_t o_sa = 0, o_aa = o_sa + sizeof(SearchArgs) * nlinks, o_fd = o_aa + sizeof(AccumArgs) * nlinks,
               o_sb = o_fd + sizeof(FinalDesc) * nlinks, o_ab = o_sb + sizeof(uint32_t) * (size_t)(nlinks + ngroups),
               o_mv = ((o_ab + sizeof(uint32_t) * (size_t)(nlinks + ngroups) + 127) / 128) * 128,
               total = o_mv + nmat_max * sizeof(Mat4);
  if ((rc = c->multi_args.ensure(total))) return rc;
  if ((rc = stage_reserve(c, total))) return rc;
  std::vector<char> tab(total, 0);
  Mat4* hmv = reinterpret_cast<Mat4*>(tab.data() + o_mv);
  const Mat4* dmv = reinterpret_cast<const Mat4*>(static_cast<char*>(c->multi_args.p) + o_mv);
  size_t nmat = 0;
  SearchArgs* hsa = reinterpret_cast<SearchArgs*>(tab.data() + o_sa);
  AccumArgs* haa = reinterpret_cast<AccumArgs*>(tab.data() + o_aa);
  FinalDesc* hfd = reinterpret_cast<FinalDesc*>(tab.data() + o_fd);
  uint32_t* hsb = reinterpret_cast<uint32_t*>(tab.data() + o_sb);
  uint32_t* hab = reinterpret_cast<uint32_t*>(tab.data() + o_ab);
  std::vector<uint32_t> s_total(ngroups), a_total(ngroups);
  struct Held { Lane* sl; uint64_t tree, scan; size_t n; };
  std::vector<Held> held;
  if (c->counting) { for (int i = 0; i < nlinks; i++) c->counted_queries += second[i]->N; }
  for (int gi = 0; gi < ngroups; gi++) {
    const int l0 = gi * G, l1 = std::min(nlinks, l0 + G);
    uint32_t sb = 0, ab = 0;
    std::map<tdtk_scan*, std::pair<size_t, int>> moving;   // scans this launch moves: where their chain sits, its length
    for (int p = l0; p < l1; p++) {
      const int i = p, li = ord[p];      // i: position in the tables; li: the caller's link
      const tdtk_tree* t = first[li];
      tdtk_scan* data = second[li];
      bool owner = false;
      if (lazy && !data->pending.empty() && moving.find(data) == moving.end()) {
        // the first link of the launch that reads the scan owns its update
        moving[data] = std::make_pair(nmat, (int)data->pending.size());
        for (const Mat4& m : data->pending) hmv[nmat++] = m;
        owner = true;
      }
      const auto mv = moving.find(data);
      Lane* sl = c->slots[i - l0].get();
      const double* A16 = first_dalignxf + 16 * (size_t)li;
      Mat4 A, inv;
      std::memcpy(A.m, A16, sizeof A.m);
      m4inv(A16, inv.m);
      SearchArgs sa{};
      sa.T = t->dev;
      sa.x = data->x; sa.y = data->y; sa.z = data->z;
      sa.n = data->N; sa.inv = inv; sa.has_inv = 1; sa.maxd2 = maxd2;
      sa.kpos = sl->kpos.as<int>();
      // the previous pass of this very link left its hits here (graph-SLAM rounds repeat their links): each search starts from
      // its previous hit, a point of this tree whatever the scans have done since (k_search's warm start; same index, same d2)
      sa.warm = (link_warm && !c->count_cold && sl->k_tree == t->uid && sl->k_scan == data->uid && sl->k_n == data->N) ? 1 : 0;
      sa.margin = sa.warm ? search_margin(t, maxd2) : 0.0;
      // (what the slot will hold is written down once every launch of the call is enqueued: a call that fails on the way must
      //  not leave a slot named after hits that were never written)
      sl->k_tree = sl->k_scan = 0;
      held.push_back({sl, t->uid, data->uid, data->N});
      const int need = (int)t->info.max_depth - 1 - search_lds_depth();
      if (need > 0) { sa.ovf_m2 = sl->ovf_m2.as<double>(); sa.ovf_ref = sl->ovf_ref.as<uint32_t>(); }
      if (c->counting) sa.counters = c->d_counters.as<unsigned long long>();
      const uint32_t nb = search_multi_prepare(sa, l1 - l0, fuse_links);
      if (ordered) {
        LinkCost* lc = c->link_costs[p].get();
        sa.cost = lc->cost.as<unsigned char>();
        sa.use_cost = (lc->tree == (const void*)t && lc->scan == (const void*)data && lc->n == data->N) ? 1 : 0;
        lc->tree = t; lc->scan = data; lc->n = data->N;
      }
      if (fuse_links) { sa.fuse = 5; sa.A = A; sa.partials = sl->part.as<double>(); }
      if (mv != moving.end()) {
        // the link's waves move their slabs first: out of the scan's arrays into the link's own copy (SearchArgs::moves)
        sa.moves = dmv + mv->second.first; sa.nmoves = mv->second.second;
        sa.sx = data->x; sa.sy = data->y; sa.sz = data->z;
        if (owner) { sa.x = data->ax; sa.y = data->ay; sa.z = data->az; sa.nx = data->nx; sa.ny = data->ny; sa.nz = data->nz; }
        else { double* m = sl->moved.as<double>(); sa.x = m; sa.y = m + maxN; sa.z = m + 2 * maxN; }
      }
      hsb[i + gi] = sb; sb += nb;
      hsa[i] = sa;
      AccumArgs aa{};
      aa.T = t->dev;
      aa.x = data->x; aa.y = data->y; aa.z = data->z;
      if (mv != moving.end()) { aa.x = sa.x; aa.y = sa.y; aa.z = sa.z; }   // (k_accum_multi runs behind the search launch)
      aa.kpos = sa.kpos; aa.n = data->N; aa.A = A; aa.inv = inv;
      for (int k = 0; k < 3; k++) aa.shift[k] = shifts[3 * li + k];
      aa.partials = sl->part.as<double>();
      const uint32_t ag = accum_grid(data->N);
      hab[i + gi] = ab; ab += ag;
      haa[i] = aa;
      hfd[i].partials = aa.partials; hfd[i].out = d_out + (size_t)li * ACC_TOTAL; hfd[i].rows = fuse_links ? (int)nb : (int)ag;
      hfd[i].pad = (want == (TDTK_WANT_LUM | ACC_WANT_NO_CROSS)) ? 1 : 0;   // k_final_multi: which columns the rows fill
    }
    hsb[l1 + gi] = sb; hab[l1 + gi] = ab;
    s_total[gi] = sb; a_total[gi] = ab;
    // behind this launch the spare arrays hold the scan (the launches of the call run in this order on one stream)
    for (auto& kv : moving) {
      tdtk_scan* sc = kv.first;
      std::swap(sc->x, sc->ax); std::swap(sc->y, sc->ay); std::swap(sc->z, sc->az);
      sc->pending.clear();
      sc->npend.store(0, std::memory_order_release);
    }
  }
  void* staged = nullptr;
  if ((rc = stage_pinned(c, tab.data(), total, &staged))) return rc;
  HIPCHK(hipMemcpyAsync(c->multi_args.p, staged, total, hipMemcpyHostToDevice, s));
  char* dbase = static_cast<char*>(c->multi_args.p);
  const int cls = search_multi_class(maxN);
  // idle lanes a wave collects before it hands out new queries: 32 once a launch is many generations of waves (84 links of
  // 1M points, ordered: 8.93 -> 8.85 ms), as for single passes of 4M queries and more (refill_thresh)
  // (22 links: 2.627 ms with 16 against 2.652 with 32; 11 links 1.416 against 1.422)
  const int thresh = (G > 32 && cls == 20 && !lab_env("TDTK_REFILL_THRESH")) ? 32 : search_multi_thresh(maxN);
  for (int gi = 0; gi < ngroups; gi++) {
    const int l0 = gi * G, l1 = std::min(nlinks, l0 + G), nb = l1 - l0;
    const bool timed = (gi == ngroups - 1) && kernel_timing();   // tdtk_last_kernel_ms: the last group's search launch
    if (timed) HIPCHK(hipEventRecord(c->e0, s));
    HIPCHK(launch_search_multi(reinterpret_cast<const SearchArgs*>(dbase + o_sa) + l0,
                               reinterpret_cast<const uint32_t*>(dbase + o_sb) + l0 + gi, nb, s_total[gi], cls, thresh, c->counting, s, ordered, fuse_links));
    if (timed) { HIPCHK(hipEventRecord(c->e1, s)); c->ev_pending = true; }
    HIPCHK(launch_accum_multi(reinterpret_cast<const AccumArgs*>(dbase + o_aa) + l0,
                              reinterpret_cast<const uint32_t*>(dbase + o_ab) + l0 + gi, nb, a_total[gi], want,
                              reinterpret_cast<const FinalDesc*>(dbase + o_fd) + l0, s, fuse_links));
  }
  for (const Held& h : held) { h.sl->k_tree = h.tree; h.sl->k_scan = h.scan; h.sl->k_n = h.n; }   // (a slot used by several groups: the last one's)
  return TDTK_OK;
}

static int links_device_pass(Ctx* c, int nlinks, const tdtk_tree* const* first, const double* first_dalignxf,
                             tdtk_scan* const* second, double maxd2, unsigned want, std::vector<double>& acc,
                             std::vector<double>& shifts)
{
  hipStream_t s = c->stream;
  int rc;
  if ((rc = c->ws[WS_TMPB].ensure((size_t)nlinks * ACC_TOTAL * sizeof(double)))) return rc;
  double* d_out = c->ws[WS_TMPB].as<double>();
  shifts.assign(3 * (size_t)nlinks, 0.0);
  size_t maxN = 0;
  for (int i = 0; i < nlinks; i++) {
    if (!first[i] || !second[i]) { set_error("NULL link member"); return TDTK_EINVAL; }
    if (first[i]->device != c->device || second[i]->device != c->device) { set_error("link members on another device"); return TDTK_EINVAL; }
    maxN = std::max(maxN, second[i]->N);
  }
  // With the sums added up inside the search launch a link's sums depend on the path it takes, so the path must depend on
  // the link alone and not on its company (else a rank's share of a graph with scans of several size classes would give
  // other bits than the whole): links of big scans go through the batched launch, by refill-threshold group, whatever
  // else the call holds.
  if (nlinks > 1 && link_batch_max() > 1) {
    std::vector<int> key(nlinks);
    bool mixed = false, any = false;
    for (int i = 0; i < nlinks; i++) {
      const size_t N = second[i]->N;
      key[i] = (N > 0 && link_sums_in_search(c, want, N)) ? 100 + search_multi_thresh(N) : 0;
      mixed = mixed || key[i] != key[0];
      any = any || key[i] != 0;
    }
    if (mixed && any) {
      acc.assign((size_t)nlinks * ACC_TOTAL, 0.0);
      std::vector<char> done(nlinks, 0);
      for (int i0 = 0; i0 < nlinks; i0++) {
        if (done[i0]) continue;
        std::vector<int> idx;
        for (int i = i0; i < nlinks; i++) if (!done[i] && key[i] == key[i0]) { idx.push_back(i); done[i] = 1; }
        const int n2 = (int)idx.size();
        std::vector<const tdtk_tree*> f2(n2);
        std::vector<tdtk_scan*> s2(n2);
        std::vector<double> d2(16 * (size_t)n2), a2, sh2;
        for (int k = 0; k < n2; k++) {
          f2[k] = first[idx[k]]; s2[k] = second[idx[k]];
          std::memcpy(&d2[16 * (size_t)k], first_dalignxf + 16 * (size_t)idx[k], 16 * sizeof(double));
        }
        if ((rc = links_device_pass(c, n2, f2.data(), d2.data(), s2.data(), maxd2, want, a2, sh2))) return rc;
        for (int k = 0; k < n2; k++) {
          std::memcpy(&acc[(size_t)idx[k] * ACC_TOTAL], &a2[(size_t)k * ACC_TOTAL], ACC_TOTAL * sizeof(double));
          for (int q = 0; q < 3; q++) shifts[3 * (size_t)idx[k] + q] = sh2[3 * (size_t)k + q];
        }
      }
      return TDTK_OK;
    }
  }
  {
    const int gb = link_batch_max();
    bool ok = gb > 1 && (nlinks > 1 || link_sums_in_search(c, want, maxN)) &&
              (want == (TDTK_WANT_LUM | ACC_WANT_NO_CROSS) || (want & 7u) == TDTK_WANT_LUM || (want & 7u) == 0u);
    const int cls = search_multi_class(maxN);
    ok = ok && cls != 0;
    for (int i = 0; i < nlinks && ok; i++)      // one kernel family (and refill threshold) for the whole call
      ok = second[i]->N > 0 && search_multi_class(second[i]->N) == cls &&
           (cls != 20 || search_multi_thresh(second[i]->N) == search_multi_thresh(maxN));
    if (ok) {
      for (int i = 0; i < nlinks; i++) pass_shift(first[i], first_dalignxf + 16 * (size_t)i, &shifts[3 * (size_t)i]);
      HIPCHK(hipMemsetAsync(d_out, 0, (size_t)nlinks * ACC_TOTAL * sizeof(double), s));
      // the launch may carry out queued scan moves into the spare arrays and swap them in: until it has run no other
      // thread may find "nothing queued" on those scans and read them on its own stream -- the lock is held to the sync
      // (threads with nothing to settle never take it)
      // (with more than one context alive another host thread may queue a move on one of these scans between an unlocked
      //  test and the launch's own reading of the queues: then the lock is taken first and the test made under it)
      std::unique_lock<std::recursive_mutex> lk(g_moves_mu, std::defer_lock);
      if (g_ctx_live.load() > 1) lk.lock();
      bool moving_any = false;
      for (int i = 0; i < nlinks && !moving_any; i++) moving_any = second[i]->npend.load(std::memory_order_acquire) != 0;
      if (moving_any && !lk.owns_lock()) lk.lock();
      if ((rc = links_device_pass_batched(c, nlinks, first, first_dalignxf, second, maxd2, want, d_out, shifts, gb))) return rc;
      acc.assign((size_t)nlinks * ACC_TOTAL, 0.0);
      HIPCHK(hipMemcpyAsync(acc.data(), d_out, acc.size() * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (lk.owns_lock()) lk.unlock();
      collect_ms(c, nullptr);
      return TDTK_OK;
    }
  }
  if ((rc = scans_settle(c, second, nlinks))) return rc;     // (the passes below read the scans as they are)
  int max_lanes = 8, forced = 0;
  if (const char* e = lab_env("TDTK_LINK_LANES")) forced = std::max(1, std::min(16, atoi(e)));
  // small scans: a pass is latency-bound, 4 side by side (32 x 60K points, 41 links: 1 lane 2.35 ms, 2: 1.52, 3: 1.30,
  // 4: 1.11, 6: 1.26, 8: 1.19); big scans: 3, so the thin tail of one search and the small sum kernels overlap with
  // the next search (84 links of 1M: 1 lane 16.3 ms, 2: 13.0, 3: 12.2; more lanes than hardware queues lose, see
  // below; tools/gs_lanes_probe.py, tools/small_graph_probe.py)
  const int L = (nlinks > 1) ? std::min(nlinks, forced ? forced : std::min(max_lanes, maxN <= (size_t)262144 ? 4 : 3)) : 1;
  HIPCHK(hipMemsetAsync(d_out, 0, (size_t)nlinks * ACC_TOTAL * sizeof(double), s));
  if (L > 1) {
    // The runtime multiplexes streams onto 4 hardware queues (GPU_MAX_HW_QUEUES): streams beyond that share a queue
    // and their kernels no longer overlap -- with the null stream in use and three lanes BESIDE the context's stream,
    // 84 link passes took 15.9 ms instead of 13.2 (and four lanes lost to three in every probe).  Lane 0 is therefore
    // the context's own stream: three lanes + the null stream = four queues.
    while ((int)c->lanes.size() < L) {
      std::unique_ptr<Lane> ln(new Lane);
      if (c->lanes.empty()) { ln->s = s; ln->owns = false; }
      else HIPCHK(hipStreamCreateWithFlags(&ln->s, hipStreamNonBlocking));
      c->lanes.push_back(std::move(ln));
    }
    HIPCHK(hipStreamSynchronize(s));   // d_out is zeroed before any lane writes into it
    for (int l = 0; l < L; l++) {
      if ((rc = c->lanes[l]->kpos.ensure(maxN * sizeof(int)))) return rc;
      const size_t rows = std::max<size_t>(accum_grid(maxN), search_fused_rows(maxN, L));
      if ((rc = c->lanes[l]->part.ensure(rows * ACC_TOTAL * sizeof(double)))) return rc;
    }
  } else {
    if ((rc = c->ws[WS_KPOS].ensure(maxN * sizeof(int)))) return rc;
    if ((rc = c->ws[WS_PART].ensure((size_t)accum_grid(maxN) * ACC_TOTAL * sizeof(double)))) return rc;
  }
  for (int i = 0; i < nlinks; i++) {
    const tdtk_tree* t = first[i];
    tdtk_scan* data = second[i];
    const double* A16 = first_dalignxf + 16 * (size_t)i;
    pass_shift(t, A16, &shifts[3 * (size_t)i]);
    if (data->N == 0) continue;
    Mat4 A, inv;
    std::memcpy(A.m, A16, sizeof A.m);
    m4inv(A16, inv.m);
    Lane* ln = (L > 1) ? c->lanes[i % L].get() : nullptr;
    hipStream_t ls = ln ? ln->s : s;
    SearchArgs sa{};
    sa.side_by_side = L;
    sa.x = data->x; sa.y = data->y; sa.z = data->z;
    sa.n = data->N; sa.inv = inv; sa.has_inv = 1; sa.maxd2 = maxd2;
    sa.kpos = ln ? ln->kpos.as<int>() : c->ws[WS_KPOS].as<int>();
    // a lum6DEuler link on a lane: its 17 sums come out of the search itself (accumulated when a query retires), so
    // the pass over (x, y, z, hit, pts[hit]) that k_accum would make disappears.  Side by side the passes run ~3 waves
    // per SIMD by choice, so the 36 accumulator registers cost no occupancy here (in the single-stream ICP loop they do)
    uint32_t fused_rows = 0;
    if (ln && want == (TDTK_WANT_LUM | ACC_WANT_NO_CROSS) && search_can_fuse(sa.n) && fuse_lum_enabled()) {
      fused_rows = search_fused_rows(sa.n, L);
      sa.fuse = 2; sa.A = A;
      for (int k = 0; k < 3; k++) sa.shift[k] = shifts[3 * i + k];
      sa.partials = ln->part.as<double>();
    }
    if (ln) {
      sa.T = t->dev;
      const uint32_t grid = search_grid(sa.n);
      if ((rc = prepare_overflow_in(ln->ovf_m2, ln->ovf_ref, t, sa.n, sa))) return rc;
      if (search_uses_queue(sa.n) && (rc = ln->qc.attach(sa))) return rc;
      if (c->counting) { sa.counters = c->d_counters.as<unsigned long long>(); c->counted_queries += sa.n; }
      const bool timed = (i == nlinks - 1) && kernel_timing();   // tdtk_last_kernel_ms: this search, running beside the other lanes'
      if (timed) HIPCHK(hipEventRecord(c->e0, ls));
      HIPCHK(launch_search(sa, grid, 0, c->counting, ls));
      if (timed) { HIPCHK(hipEventRecord(c->e1, ls)); c->ev_pending = true; }
    } else {
      if ((rc = run_search(c, t, sa, 0, false, s, i == nlinks - 1))) return rc;
    }
    if (fused_rows) {
      HIPCHK(launch_final(sa.partials, fused_rows, d_out + (size_t)i * ACC_TOTAL, ls));
      continue;
    }
    AccumArgs aa{};
    aa.T = t->dev;
    aa.x = data->x; aa.y = data->y; aa.z = data->z;
    aa.kpos = sa.kpos; aa.n = data->N; aa.A = A; aa.inv = inv;
    for (int k = 0; k < 3; k++) aa.shift[k] = shifts[3 * i + k];
    aa.partials = ln ? ln->part.as<double>() : c->ws[WS_PART].as<double>();
    HIPCHK(launch_accum(aa, accum_grid(data->N), want, 0, d_out + (size_t)i * ACC_TOTAL, ls));
  }
  for (int l = 0; l < L && L > 1; l++) HIPCHK(hipStreamSynchronize(c->lanes[l]->s));
  acc.assign((size_t)nlinks * ACC_TOTAL, 0.0);
  HIPCHK(hipMemcpyAsync(acc.data(), d_out, acc.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  collect_ms(c, nullptr);
  return TDTK_OK;
}

int tdtk_links_pair_sums(int nlinks, const tdtk_tree* const* first, const double* first_dalignxf,
                         tdtk_scan* const* second, double maxd2, uint32_t want, tdtk_pair_sums* sums)
{
  if (nlinks < 0 || (nlinks && (!first || !first_dalignxf || !second || !sums))) { set_error("bad argument"); return TDTK_EINVAL; }
  if (nlinks == 0) return TDTK_OK;
  if (want & TDTK_WANT_NAPX) { set_error("NAPX needs normals: use tdtk_scan_pairs"); return TDTK_EUNSUP; }
  if (!first[0]) { set_error("NULL link member"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(first[0]->device, &c);
  if (rc) return rc;
  std::vector<double> acc, shifts;
  if ((rc = links_device_pass(c, nlinks, first, first_dalignxf, second, maxd2, want, acc, shifts))) return rc;
  for (int i = 0; i < nlinks; i++)
    finish_sums(acc.data() + (size_t)i * ACC_TOTAL, shifts.data() + 3 * i, second[i]->N, want, sums + i);
  return TDTK_OK;
}

// ---- batched links + native pose update (graph-SLAM inner loop without per-link round trips) ----
int tdtk_lum_links(int nlinks, const tdtk_tree* const* first, const double* first_dalignxf,
                   tdtk_scan* const* second, double maxd2, double* C, double* CD, uint64_t* m_out, double* ss_out)
{
  if (nlinks < 0 || (nlinks && (!first || !first_dalignxf || !second || !C || !CD))) { set_error("bad argument"); return TDTK_EINVAL; }
  if (nlinks == 0) return TDTK_OK;
  if (!first[0]) { set_error("NULL link member"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(first[0]->device, &c);
  if (rc) return rc;
  std::vector<double> acc, shifts;
  // n, sum |delta|^2 and the 15 LUM sums are all a link's block needs
  if ((rc = links_device_pass(c, nlinks, first, first_dalignxf, second, maxd2, TDTK_WANT_LUM | ACC_WANT_NO_CROSS, acc, shifts))) return rc;
  for (int i = 0; i < nlinks; i++) {
    double* Ci = C + 36 * (size_t)i;
    double* CDi = CD + 6 * (size_t)i;
    std::memset(Ci, 0, 36 * sizeof(double));
    std::memset(CDi, 0, 6 * sizeof(double));
    const double* a = acc.data() + (size_t)i * ACC_TOTAL;
    const uint64_t m = (uint64_t)(a[ACC_N] + 0.5);
    if (m_out) m_out[i] = m;
    if (ss_out) ss_out[i] = 0.0;
    if (m <= 2) continue;
    const double* L = a + ACC_L;
    const double* MZ = L + 9;
    double MM[36], D[6];
    if ((rc = lum_normal_system(m, L, MM, D))) return rc;
    double dmz = 0.0;
    for (int r = 0; r < 6; r++) dmz += D[r] * MZ[r];
    // sum |delta - A(u) D|^2 = sum|delta|^2 - 2 D.MZ + D.MM.D = sum|delta|^2 - D.MZ for MM D = MZ
    double ss = (a[ACC_SUM] - dmz) / (2.0 * (double)m - 3.0);
    if (ss_out) ss_out[i] = ss;
    if (ss < 0.0000000000001) continue;
    ss = 1.0 / ss;
    for (int k = 0; k < 36; k++) Ci[k] = MM[k] * ss;
    for (int k = 0; k < 6; k++) CDi[k] = MZ[k] * ss;
  }
  return TDTK_OK;
}

}  // extern "C"
