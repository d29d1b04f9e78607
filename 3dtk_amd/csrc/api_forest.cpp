// The dynamic kd-forest (BkdTree): the handle, the insert plan, merges over the device build, the remove pass and the three
// queries of forest.hip.  The rules of every operation are in forest_lane.h.
#include "api_internal.h"
#include "query.h"
#include "forest.h"

using namespace tdtk;

namespace tdtk {

// ---- the insert plan (host only) ---------------------------------------------------------------------------------------
// BkdTree::insert (bkd.cc:148-201) m times, over segment lists instead of points: a point goes to the buffer; when the
// buffer holds exactly b points the slots are walked from 0, the first empty one (or a new one behind the last) takes one
// tree over everything in front of it plus the buffer, and those are emptied.  "Empty" is a live count of 0: a slot a merge
// consumed, one the constructor left in front of its tree, or one whose last point was removed.
static void seg_append(std::vector<ForestSeg>& v, const ForestSeg& s)
{
  if (s.kind == FOREST_SEG_NEW && !v.empty() && v.back().kind == FOREST_SEG_NEW && v.back().b == s.a) v.back().b = s.b;
  else v.push_back(s);
}

void forest_plan(const std::vector<uint64_t>& counts, uint64_t fill, uint64_t bucket, uint64_t m, ForestPlan& out)
{
  std::vector<std::vector<ForestSeg>>& S = out.segs;
  std::vector<uint64_t>& C = out.counts;
  C = counts;
  S.assign(C.size(), {});
  for (size_t s = 0; s < C.size(); s++)
    if (C[s]) S[s].push_back({FOREST_SEG_SLOT, (int64_t)s, (int64_t)C[s]});
  std::vector<ForestSeg> buf;
  if (fill) buf.push_back({FOREST_SEG_BUFFER, 0, (int64_t)fill});
  uint64_t bfill = fill, pos = 0;
  out.keeps_buffer = true;
  out.merges = 0;
  while (pos < m) {
    const uint64_t take = std::min(m - pos, bucket - bfill);
    seg_append(buf, {FOREST_SEG_NEW, (int64_t)pos, (int64_t)(pos + take)});
    bfill += take; pos += take;
    if (bfill != bucket) break;
    size_t i = 0;
    uint64_t total = bfill;
    std::vector<ForestSeg> segs;
    for (; i < S.size() && C[i]; i++) {
      for (const ForestSeg& g : S[i]) seg_append(segs, g);
      total += C[i];
      S[i].clear(); C[i] = 0;
    }
    if (i == S.size()) { S.emplace_back(); C.push_back(0); }
    for (const ForestSeg& g : buf) seg_append(segs, g);
    S[i] = std::move(segs); C[i] = total;
    buf.clear(); bfill = 0;
    out.keeps_buffer = false;
    out.merges++;
  }
  // The order in which a merged slot's points reach the builder is free (only the set is the reference's): the old slots in
  // ascending order, the old buffer, then the new points in insertion order -- which are one range per slot once sorted, where
  // the history of the merges leaves thousands of pieces (3 750 for 100 000 points at b = 20), each a launch of its own.
  for (std::vector<ForestSeg>& v : S) {
    std::stable_sort(v.begin(), v.end(), [](const ForestSeg& x, const ForestSeg& y) {
      auto rank = [](const ForestSeg& g) { return g.kind == FOREST_SEG_SLOT ? 0 : g.kind == FOREST_SEG_BUFFER ? 1 : 2; };
      return rank(x) != rank(y) ? rank(x) < rank(y) : x.a < y.a;
    });
    std::vector<ForestSeg> w;
    for (const ForestSeg& g : v) seg_append(w, g);
    v = std::move(w);
  }
  out.buf_a = out.buf_b = m;
  for (const ForestSeg& g : buf)
    if (g.kind == FOREST_SEG_NEW) { out.buf_a = (uint64_t)g.a; out.buf_b = (uint64_t)g.b; }
}

}  // namespace tdtk

// ---- the handle ----------------------------------------------------------------------------------------------------------
// The trees of a forest are private to it: built by tree_from_device_points and left as built -- no padded buckets, no
// KdHot / KdFat records (only the ICP search reads those), never handed out as tdtk_tree.
struct tdtk_forest {
  int device = 0;
  int bucket = 0;
  int64_t next_id = 0;                                  // the running insertion counter
  std::vector<std::unique_ptr<tdtk_tree>> slots;        // null: empty
  std::vector<uint64_t> live;                           // live points per slot
  void* d_buf = nullptr;                                // the buffer on the device, `bucket` KdPoints
  std::vector<KdPoint> h_buf;                           // ... and its mirror, in insertion order
  bool has_box = false;
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};          // every point ever inserted: what the queries are binned on
  tdtk_tree proxy;                                      // query_prepare's stand-in: carries the deepest slot's depth
  DevBuf ids, flags, offs, scan_tmp, ctl, res, cand_c, cand_p;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};       // around the gathers and the build of one slot (tdtk_forest_last_insert)
  double last_insert[6] = {0, 0, 0, 0, 0, 0};
  tdtk_forest() = default;
  tdtk_forest(const tdtk_forest&) = delete;
  tdtk_forest& operator=(const tdtk_forest&) = delete;
  ~tdtk_forest()
  {
    (void)hipSetDevice(device);
    if (d_buf) pool_free(d_buf);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  uint64_t size() const
  {
    uint64_t n = h_buf.size();
    for (uint64_t c : live) n += c;
    return n;
  }
};

namespace {

int forest_check_points(const double* xyz, size_t n)
{
  for (size_t i = 0; i < 3 * n; i++)
    if (!std::isfinite(xyz[i])) { set_error("non-finite coordinate"); return TDTK_EINVAL; }
  return TDTK_OK;
}

void forest_grow_box(tdtk_forest* f, const double* xyz, size_t n)
{
  for (size_t i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) {
      const double v = xyz[3 * i + a];
      if (!f->has_box || v < f->lo[a]) f->lo[a] = v;
      if (!f->has_box || v > f->hi[a]) f->hi[a] = v;
      if (a == 2) f->has_box = true;
    }
}

// one tree over the cnt points sitting in c->ws[WS_TMPA], their ids in `ids` (null: 0 .. cnt-1)
int forest_build_slot(Ctx* c, tdtk_forest* f, size_t cnt, const int32_t* ids, std::unique_ptr<tdtk_tree>& out, hipEvent_t done = nullptr)
{
  int rc;
  std::unique_ptr<tdtk_tree> t(new tdtk_tree);
  t->device = f->device; t->M = cnt; t->bucket = f->bucket; t->Mp = cnt;
  if ((rc = tree_check_args(cnt, f->bucket))) return rc;
  if ((rc = tree_from_device_points(c, t.get(), cnt, f->bucket, now_ms()))) return rc;
  t->dev.nodes = static_cast<const KdNode*>(t->d_nodes);
  t->dev.pts = static_cast<const KdPoint*>(t->d_pts);
  t->dev.leaf_tab = static_cast<const LeafEntry*>(t->d_leaf);
  t->dev.node_r = static_cast<const double*>(t->d_r);
  t->dev.cmask = (t->dev.cb >= 32) ? 0xFFFFFFFFu : ((1u << t->dev.cb) - 1u);
  t->info.n_points = cnt;
  HIPCHK(launch_forest_relabel(static_cast<KdPoint*>(t->d_pts), cnt, ids, c->stream));
  if (done) HIPCHK(hipEventRecord(done, c->stream));
  // (the build's side streams are joined into the context's stream: behind this the points in WS_TMPA are free again)
  HIPCHK(hipStreamSynchronize(c->stream));
  out = std::move(t);
  return TDTK_OK;
}

int forest_upload_buffer(Ctx* c, tdtk_forest* f)
{
  if (f->h_buf.empty()) return TDTK_OK;
  HIPCHK(hipMemcpyAsync(f->d_buf, f->h_buf.data(), f->h_buf.size() * sizeof(KdPoint), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TDTK_OK;
}

void forest_fill_args(const tdtk_forest* f, ForestArgs& a)
{
  a.buf = static_cast<KdPoint*>(f->d_buf);
  a.nbuf = (uint32_t)f->h_buf.size();
  a.nslots = (int)f->slots.size();
  for (int s = 0; s < a.nslots; s++) {
    const tdtk_tree* t = f->slots[s].get();
    ForestSlot& d = a.slot[s];
    d = ForestSlot{};
    if (!t) continue;
    d.nodes = t->dev.nodes; d.pts = static_cast<KdPoint*>(t->d_pts); d.leaf_tab = t->dev.leaf_tab;
    d.root_ref = t->dev.root_ref; d.cb = t->dev.cb; d.cmask = t->dev.cmask; d.n = (uint32_t)t->M;
  }
}

// the K points at q [K][3] uploaded and binned on the forest's box, the stack overflow area for the deepest slot, the table
int forest_query_begin(Ctx* c, tdtk_forest* f, const double* q, size_t K, ForestArgs& a)
{
  int rc;
  if ((rc = c->ws[WS_TMPA].ensure(3 * K * sizeof(double)))) return rc;
  double* dq = c->ws[WS_TMPA].as<double>();
  HIPCHK(hipMemcpyAsync(dq, q, 3 * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
  uint32_t depth = 0;
  for (const auto& t : f->slots)
    if (t) depth = std::max(depth, t->info.max_depth);
  f->proxy.info.max_depth = depth;
  const double box[6] = {f->lo[0], f->lo[1], f->lo[2], f->hi[0], f->hi[1], f->hi[2]};
  a = ForestArgs{};
  if ((rc = query_prepare(c, &f->proxy, dq, K, a.q, nullptr, box))) return rc;
  forest_fill_args(f, a);
  return TDTK_OK;
}

int forest_check(const tdtk_forest* f, const double* q, size_t K)
{
  if (!f || (!q && K)) { set_error("NULL argument"); return TDTK_EINVAL; }
  return TDTK_OK;
}

}  // namespace

extern "C" {

int tdtk_forest_create(int bucket, int device, tdtk_forest** out)
{
  if (!out) { set_error("out is NULL"); return TDTK_EINVAL; }
  *out = nullptr;
  if (bucket < 1) { set_error("bucket size must be >= 1"); return TDTK_EINVAL; }
  Ctx* c;
  int rc = get_ctx(device, &c);
  if (rc) return rc;
  std::unique_ptr<tdtk_forest> f(new tdtk_forest);
  f->device = device; f->bucket = bucket; f->proxy.device = device;
  HIPCHK(handle_malloc(&f->d_buf, (size_t)bucket * sizeof(KdPoint)));
  for (hipEvent_t& e : f->ev) HIPCHK(hipEventCreate(&e));
  *out = f.release();
  return TDTK_OK;
}

// BkdTree(pts, n, b) (bkd.cc:11-33): nrtrees = max(1.0, ceil(log2(n / b))) with n / b an integer division -- n < b gives
// log2(0) and one slot --, nrtrees - 1 empty slots and behind them one tree over all n points
int tdtk_forest_create_from_points(const double* xyz, size_t n, int bucket, int device, tdtk_forest** out)
{
  if (!out) { set_error("out is NULL"); return TDTK_EINVAL; }
  *out = nullptr;
  if (!xyz || n == 0) { set_error("cannot create kdtree with zero points"); return TDTK_EINVAL; }
  if (n > 0x7FFFFFFFull) { set_error("too many points for 32-bit ids"); return TDTK_EINVAL; }
  int rc;
  if ((rc = forest_check_points(xyz, n))) return rc;
  tdtk_forest* f = nullptr;
  if ((rc = tdtk_forest_create(bucket, device, &f))) return rc;
  std::unique_ptr<tdtk_forest> hold(f);
  Ctx* c;
  if ((rc = get_ctx(device, &c))) return rc;
  const int nrtrees = (int)std::max(1.0, std::ceil(std::log2((double)(n / (size_t)bucket))));
  if (nrtrees > FOREST_MAX_SLOTS) { set_error("more than 32 slots"); return TDTK_EUNSUP; }
  if ((rc = c->ws[WS_TMPA].ensure(3 * n * sizeof(double)))) return rc;
  HIPCHK(hipMemcpyAsync(c->ws[WS_TMPA].p, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  std::unique_ptr<tdtk_tree> t;
  if ((rc = forest_build_slot(c, f, n, nullptr, t))) return rc;
  f->slots.resize(nrtrees);
  f->live.assign(nrtrees, 0);
  f->slots[nrtrees - 1] = std::move(t);
  f->live[nrtrees - 1] = n;
  f->next_id = (int64_t)n;
  forest_grow_box(f, xyz, n);
  *out = hold.release();
  return TDTK_OK;
}

void tdtk_forest_destroy(tdtk_forest* f)
{
  if (!f) return;
  wait_deferred(f->device);
  delete f;
}

// m single inserts in one call (forest_plan): every slot of the final layout that changed is gathered and built once
int tdtk_forest_insert(tdtk_forest* f, const double* xyz, size_t m, int32_t* first_id_out)
{
  if (!f || (!xyz && m)) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (first_id_out) *first_id_out = (int32_t)f->next_id;
  if (m == 0) return TDTK_OK;
  int rc;
  if ((rc = forest_check_points(xyz, m))) return rc;
  if ((uint64_t)f->next_id + m > 0x7FFFFFFFull) { set_error("too many points for 32-bit ids"); return TDTK_EINVAL; }
  Ctx* c;
  if ((rc = get_ctx(f->device, &c))) return rc;
  const double t0 = now_ms();
  ForestPlan plan;
  forest_plan(f->live, f->h_buf.size(), (uint64_t)f->bucket, m, plan);
  const double t_plan = now_ms() - t0;
  double gather_ms = 0.0, build_ms = 0.0, slots_built = 0.0;
  if (plan.counts.size() > (size_t)FOREST_MAX_SLOTS) { set_error("more than 32 slots"); return TDTK_EUNSUP; }
  for (uint64_t cnt : plan.counts)
    if ((rc = tree_check_args(cnt, f->bucket))) return rc;
  hipStream_t s = c->stream;
  const int32_t first_id = (int32_t)f->next_id;
  const double* d_new = nullptr;
  std::vector<std::unique_ptr<tdtk_tree>> built(plan.counts.size());
  std::vector<char> rebuilt(plan.counts.size(), 0);
  if (plan.merges) {
    if ((rc = c->ws[WS_TMPB].ensure(3 * m * sizeof(double)))) return rc;
    HIPCHK(hipMemcpyAsync(c->ws[WS_TMPB].p, xyz, 3 * m * sizeof(double), hipMemcpyHostToDevice, s));
    d_new = c->ws[WS_TMPB].as<double>();
  }
  for (size_t j = 0; j < plan.counts.size(); j++) {
    const std::vector<ForestSeg>& segs = plan.segs[j];
    const uint64_t cnt = plan.counts[j];
    if (cnt == 0) continue;
    if (segs.size() == 1 && segs[0].kind == FOREST_SEG_SLOT && segs[0].a == (int64_t)j) continue;    // untouched
    rebuilt[j] = 1;
    if ((rc = c->ws[WS_TMPA].ensure(3 * cnt * sizeof(double)))) return rc;
    if ((rc = f->ids.ensure(cnt * sizeof(int32_t)))) return rc;
    double* d_xyz = c->ws[WS_TMPA].as<double>();
    int32_t* d_ids = f->ids.as<int32_t>();
    size_t base = 0;
    HIPCHK(hipEventRecord(f->ev[0], s));
    for (const ForestSeg& g : segs) {
      if (g.kind == FOREST_SEG_NEW) {
        HIPCHK(launch_forest_copy_new(d_new, (size_t)g.a, (size_t)g.b, first_id, d_xyz, d_ids, base, s));
        base += (size_t)(g.b - g.a);
      } else if (g.kind == FOREST_SEG_BUFFER) {
        HIPCHK(launch_forest_copy_points(static_cast<const KdPoint*>(f->d_buf), (size_t)g.b, d_xyz, d_ids, base, s));
        base += (size_t)g.b;
      } else {
        const tdtk_tree* t = f->slots[(size_t)g.a].get();
        const KdPoint* pts = static_cast<const KdPoint*>(t->d_pts);
        if ((uint64_t)g.b == t->M) {      // nothing was removed from it
          HIPCHK(launch_forest_copy_points(pts, t->M, d_xyz, d_ids, base, s));
        } else {                          // the live ones, in storage order
          const size_t n1 = t->M + 1, tmpb = scan_u32_temp_bytes(n1);
          if ((rc = f->flags.ensure(n1 * sizeof(uint32_t)))) return rc;
          if ((rc = f->offs.ensure(n1 * sizeof(uint32_t)))) return rc;
          if ((rc = f->scan_tmp.ensure(tmpb + 256))) return rc;
          HIPCHK(launch_forest_live_flags(pts, t->M, f->flags.as<uint32_t>(), s));
          HIPCHK(launch_scan_u32(f->flags.as<uint32_t>(), f->offs.as<uint32_t>(), n1, f->scan_tmp.p, tmpb, s));
          HIPCHK(launch_forest_compact_points(pts, t->M, f->offs.as<uint32_t>(), d_xyz, d_ids, base, s));
        }
        base += (size_t)g.b;
      }
    }
    if (base != cnt) { set_error("forest plan: a slot's segments do not add up"); return TDTK_EDEVICE; }
    HIPCHK(hipEventRecord(f->ev[1], s));
    if ((rc = forest_build_slot(c, f, cnt, d_ids, built[j], f->ev[2]))) return rc;
    float g_ms = 0.f, b_ms = 0.f;
    HIPCHK(hipEventElapsedTime(&g_ms, f->ev[0], f->ev[1]));
    HIPCHK(hipEventElapsedTime(&b_ms, f->ev[1], f->ev[2]));
    gather_ms += g_ms; build_ms += b_ms; slots_built += 1.0;
  }
  // nothing has failed: the new layout takes over, the consumed trees go back to the pool
  HIPCHK(hipStreamSynchronize(s));
  f->slots.resize(plan.counts.size());
  for (size_t j = 0; j < plan.counts.size(); j++) {
    if (rebuilt[j]) f->slots[j] = std::move(built[j]);
    else if (plan.counts[j] == 0) f->slots[j].reset();
  }
  f->live = plan.counts;
  if (!plan.keeps_buffer) f->h_buf.clear();
  for (uint64_t i = plan.buf_a; i < plan.buf_b; i++) {
    KdPoint p;
    p.x = xyz[3 * i]; p.y = xyz[3 * i + 1]; p.z = xyz[3 * i + 2];
    p.orig = first_id + (int32_t)i; p.pad = FOREST_UNCLAIMED;
    f->h_buf.push_back(p);
  }
  if ((rc = forest_upload_buffer(c, f))) return rc;
  f->next_id += (int64_t)m;
  forest_grow_box(f, xyz, m);
  const double ms[6] = {t_plan, gather_ms, build_ms, now_ms() - t0, slots_built, (double)plan.merges};
  std::memcpy(f->last_insert, ms, sizeof ms);
  return TDTK_OK;
}

// the last tdtk_forest_insert of f, ms: the plan (host clock), the gathers and the builds of the slots it built (HIP events, summed
// over the slots), the call end to end (host clock); then the number of slots built and of merges they stand for
int tdtk_forest_last_insert(const tdtk_forest* f, double out6[6])
{
  if (!f || !out6) { set_error("NULL argument"); return TDTK_EINVAL; }
  std::memcpy(out6, f->last_insert, sizeof f->last_insert);
  return TDTK_OK;
}

// BkdTree::remove for the m points at xyz, as if applied in order (forest_lane.h: the device rule): removed_id_out [m], the
// id that went or -1
int tdtk_forest_remove(tdtk_forest* f, const double* xyz, size_t m, int32_t* removed_id_out)
{
  if (!f || ((!xyz || !removed_id_out) && m)) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (m == 0) return TDTK_OK;
  if (m > 0x7FFFFFFEull) { set_error("too many requests"); return TDTK_EINVAL; }
  int rc;
  if ((rc = forest_check_points(xyz, m))) return rc;
  if (f->size() == 0) { std::fill(removed_id_out, removed_id_out + m, -1); return TDTK_OK; }
  Ctx* c;
  if ((rc = get_ctx(f->device, &c))) return rc;
  hipStream_t s = c->stream;
  ForestArgs a;
  if ((rc = forest_query_begin(c, f, xyz, m, a))) return rc;
  constexpr size_t NCTL = 2 + 1 + FOREST_MAX_SLOTS;
  if ((rc = f->ctl.ensure(NCTL * sizeof(uint32_t)))) return rc;
  if ((rc = f->res.ensure(m * sizeof(int32_t)))) return rc;
  if ((rc = f->cand_c.ensure(m * sizeof(int32_t)))) return rc;
  if ((rc = f->cand_p.ensure(m * sizeof(uint32_t)))) return rc;
  a.ctl = f->ctl.as<uint32_t>(); a.res = f->res.as<int32_t>();
  a.cand_c = f->cand_c.as<int32_t>(); a.cand_p = f->cand_p.as<uint32_t>();
  HIPCHK(hipMemsetAsync(a.ctl, 0, NCTL * sizeof(uint32_t), s));
  std::fill(removed_id_out, removed_id_out + m, -2);                // every request starts pending
  HIPCHK(hipMemcpyAsync(a.res, removed_id_out, m * sizeof(int32_t), hipMemcpyHostToDevice, s));
  uint32_t ctl[NCTL];
  for (size_t round = 0; round <= m; round++) {
    HIPCHK(launch_forest_remove_round(a, s));
    HIPCHK(hipMemcpyAsync(ctl, a.ctl, sizeof ctl, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctl[1] == 0) break;
  }
  if (ctl[1] != 0) { set_error("forest remove: requests left pending"); return TDTK_EDEVICE; }
  HIPCHK(hipMemcpyAsync(removed_id_out, a.res, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  // the buffer closes up in order; a tree whose count reaches 0 becomes an empty slot
  if (ctl[2]) {
    std::vector<KdPoint> got(f->h_buf.size());
    HIPCHK(hipMemcpy(got.data(), f->d_buf, got.size() * sizeof(KdPoint), hipMemcpyDeviceToHost));
    f->h_buf.clear();
    for (const KdPoint& p : got)
      if (p.orig >= 0) f->h_buf.push_back(p);
    if ((rc = forest_upload_buffer(c, f))) return rc;
  }
  for (size_t sl = 0; sl < f->slots.size(); sl++) {
    const uint64_t gone = ctl[3 + sl];
    if (!gone) continue;
    f->live[sl] = (gone >= f->live[sl]) ? 0 : f->live[sl] - gone;
    if (f->live[sl] == 0) f->slots[sl].reset();
  }
  return TDTK_OK;
}

// counts [FOREST_MAX_SLOTS] (the first *nslots written), the buffer's fill, size(); table_mask: bit s set when slot s's tree
// keeps its leaves in a table (all nullable)
int tdtk_forest_info(const tdtk_forest* f, int* nslots, uint64_t* counts, uint64_t* buffer_fill, uint64_t* size, uint32_t* table_mask)
{
  if (!f) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (nslots) *nslots = (int)f->slots.size();
  if (counts)
    for (size_t s = 0; s < f->live.size(); s++) counts[s] = f->live[s];
  if (buffer_fill) *buffer_fill = f->h_buf.size();
  if (size) *size = f->size();
  if (table_mask) {
    *table_mask = 0;
    for (size_t s = 0; s < f->slots.size(); s++)
      if (f->slots[s] && f->slots[s]->d_leaf) *table_mask |= 1u << s;
  }
  return TDTK_OK;
}

// the live points of slot `slot` in storage order, or of the buffer (slot -1) in insertion order: ids [cap], xyz [cap][3]
// (nullable each), *n their number (written also when cap is too small: TDTK_EINVAL then)
int tdtk_forest_collect(const tdtk_forest* f, int slot, int32_t* ids, double* xyz, size_t cap, uint64_t* n)
{
  if (!f || !n) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (slot < -1 || slot >= (int)f->slots.size()) { set_error("no such slot"); return TDTK_EINVAL; }
  std::vector<KdPoint> got;
  if (slot < 0) got = f->h_buf;
  else if (f->slots[slot]) {
    Ctx* c;
    int rc;
    if ((rc = get_ctx(f->device, &c))) return rc;
    got.resize(f->slots[slot]->M);
    HIPCHK(hipMemcpy(got.data(), f->slots[slot]->d_pts, got.size() * sizeof(KdPoint), hipMemcpyDeviceToHost));
  }
  uint64_t k = 0;
  for (const KdPoint& p : got) k += p.orig >= 0;
  *n = k;
  if (k > cap) { set_error("tdtk_forest_collect: " + std::to_string(k) + " points, capacity " + std::to_string(cap)); return TDTK_EINVAL; }
  k = 0;
  for (const KdPoint& p : got) {
    if (p.orig < 0) continue;
    if (ids) ids[k] = p.orig;
    if (xyz) { xyz[3 * k] = p.x; xyz[3 * k + 1] = p.y; xyz[3 * k + 2] = p.z; }
    k++;
  }
  return TDTK_OK;
}

int tdtk_forest_find_closest(tdtk_forest* f, const double* q, size_t K, double maxdist2, int32_t* idx, double* d2)
{
  int rc;
  if ((rc = forest_check(f, q, K))) return rc;
  if (!idx && K) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (K == 0) return TDTK_OK;
  if (f->size() == 0) {
    std::fill(idx, idx + K, -1);
    if (d2) std::fill(d2, d2 + K, -1.0);
    return TDTK_OK;
  }
  Ctx* c;
  if ((rc = get_ctx(f->device, &c))) return rc;
  hipStream_t s = c->stream;
  ForestArgs a;
  if ((rc = forest_query_begin(c, f, q, K, a))) return rc;
  if ((rc = c->ws[WS_IDX].ensure(K * sizeof(int32_t)))) return rc;
  if (d2 && (rc = c->ws[WS_TMPB].ensure(K * sizeof(double)))) return rc;
  a.q.r2 = maxdist2;
  a.q.idx = c->ws[WS_IDX].as<int32_t>();
  a.q.d2 = d2 ? c->ws[WS_TMPB].as<double>() : nullptr;
  HIPCHK(launch_forest_find_closest(a, s));
  HIPCHK(hipMemcpyAsync(idx, a.q.idx, K * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (d2) HIPCHK(hipMemcpyAsync(d2, a.q.d2, K * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return TDTK_OK;
}

int tdtk_forest_knn(tdtk_forest* f, const double* q, size_t K, int k, int32_t* idx, double* d2)
{
  int rc;
  if ((rc = forest_check(f, q, K))) return rc;
  if (!idx && K) { set_error("NULL argument"); return TDTK_EINVAL; }
  if ((rc = knn_check_k(k))) return rc;
  if (K == 0) return TDTK_OK;
  const size_t L = K * (size_t)k;
  if (f->size() == 0) {
    std::fill(idx, idx + L, -1);
    if (d2) std::fill(d2, d2 + L, -1.0);
    return TDTK_OK;
  }
  Ctx* c;
  if ((rc = get_ctx(f->device, &c))) return rc;
  hipStream_t s = c->stream;
  ForestArgs a;
  if ((rc = forest_query_begin(c, f, q, K, a))) return rc;
  if ((rc = c->ws[WS_IDX].ensure(L * sizeof(int32_t)))) return rc;
  if (d2 && (rc = c->ws[WS_TMPB].ensure(L * sizeof(double)))) return rc;
  a.q.k = k;
  a.q.idx = c->ws[WS_IDX].as<int32_t>();
  a.q.d2 = d2 ? c->ws[WS_TMPB].as<double>() : nullptr;
  HIPCHK(launch_forest_knn(a, s));
  HIPCHK(hipMemcpyAsync(idx, a.q.idx, L * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (d2) HIPCHK(hipMemcpyAsync(d2, a.q.d2, L * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return TDTK_OK;
}

// count walk, scan, fill walk, as tdtk_fixed_range_search: offsets [K + 1] and *total always; idx / d2 [cap] when they hold it
int tdtk_forest_fixed_range(tdtk_forest* f, const double* q, size_t K, double sqRad2, uint64_t* offsets, int32_t* idx, double* d2,
                            size_t cap, uint64_t* total)
{
  int rc;
  if ((rc = forest_check(f, q, K))) return rc;
  if (!offsets || !total) { set_error("NULL argument"); return TDTK_EINVAL; }
  offsets[0] = 0; *total = 0;
  if (K == 0) return TDTK_OK;
  if (f->size() == 0) { std::fill(offsets, offsets + K + 1, 0); return TDTK_OK; }
  Ctx* c;
  if ((rc = get_ctx(f->device, &c))) return rc;
  hipStream_t s = c->stream;
  ForestArgs a;
  if ((rc = forest_query_begin(c, f, q, K, a))) return rc;
  a.q.r2 = sqRad2;
  auto count = [&]() { HIPCHK(launch_forest_range_count(a, s)); return TDTK_OK; };
  auto fill = [&]() { HIPCHK(launch_forest_range_fill(a, s)); return TDTK_OK; };
  return list_walks(c, "tdtk_forest_fixed_range", "neighbours", a.q, false, count, fill, offsets, idx, d2, cap, total);
}

// The insert plan, host only: counts [nslots] and fill (< bucket) before, m points inserted.  counts_out [FOREST_MAX_SLOTS] (the
// first *nslots_out written), segs [cap_segs][4] = { final slot, kind, a, b } (0: the live points of old slot a, b of them;
// 1: new points [a, b); 2: the old buffer, b points), *nsegs their number, buf_out = { old buffer kept (0 / 1), a, b }: the
// final buffer is the old one (if kept) followed by the new points [a, b); *merges: the merges simulated
int tdtk_forest_plan(const uint64_t* counts, int nslots, uint64_t fill, int bucket, uint64_t m, int* nslots_out, uint64_t* counts_out,
                     int64_t* segs, size_t cap_segs, size_t* nsegs, uint64_t buf_out[3], uint64_t* merges)
{
  if ((!counts && nslots) || !nslots_out || !counts_out || !nsegs || !buf_out) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (nslots < 0 || nslots > FOREST_MAX_SLOTS || bucket < 1 || fill >= (uint64_t)bucket) { set_error("tdtk_forest_plan: invalid state"); return TDTK_EINVAL; }
  ForestPlan plan;
  forest_plan(std::vector<uint64_t>(counts, counts + nslots), fill, (uint64_t)bucket, m, plan);
  if (plan.counts.size() > (size_t)FOREST_MAX_SLOTS) { set_error("more than 32 slots"); return TDTK_EUNSUP; }
  *nslots_out = (int)plan.counts.size();
  size_t k = 0;
  for (size_t j = 0; j < plan.counts.size(); j++) {
    counts_out[j] = plan.counts[j];
    for (const ForestSeg& g : plan.segs[j]) {
      if (k < cap_segs && segs) { segs[4 * k] = (int64_t)j; segs[4 * k + 1] = g.kind; segs[4 * k + 2] = g.a; segs[4 * k + 3] = g.b; }
      k++;
    }
  }
  *nsegs = k;
  buf_out[0] = plan.keeps_buffer ? 1 : 0; buf_out[1] = plan.buf_a; buf_out[2] = plan.buf_b;
  if (merges) *merges = plan.merges;
  if (k > cap_segs) { set_error("tdtk_forest_plan: " + std::to_string(k) + " segments, capacity " + std::to_string(cap_segs)); return TDTK_EINVAL; }
  return TDTK_OK;
}

}  // extern "C"
