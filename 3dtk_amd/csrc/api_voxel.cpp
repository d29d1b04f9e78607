// The voxel-grid entry points: tdtk_voxel_walk and tdtk_peopleremover (kernels: voxel.hip, per-lane code: voxel_lane.h).
#include "api_internal.h"
#include "query.h"
#include "voxel.h"

using namespace tdtk;

namespace {

// device memory of one call, carved out of one workspace
struct Bump {
  char* base = nullptr;
  size_t off = 0;
  template <class T> T* take(size_t count)
  {
    T* p = reinterpret_cast<T*>(base + off);
    off += (count * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
};

struct Events {
  hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool ok = true;
  Events() { for (auto& x : e) if (hipEventCreate(&x) != hipSuccess) { x = nullptr; ok = false; } }
  ~Events() { for (auto& x : e) if (x) (void)hipEventDestroy(x); }
};

thread_local double t_vox_ms[4] = {0.0, 0.0, 0.0, 0.0};

int vox_input_error(unsigned long long bits, double vs)
{
  if (bits & VOX_ERR_NONFINITE) { set_error("non-finite coordinate"); return TDTK_EINVAL; }
  if (bits & VOX_ERR_RANGE) {
    set_error("a coordinate lies outside the packable voxel range: |x / voxel_size| must stay below " +
              std::to_string((long long)VOX_LIMIT) + " (voxel_size " + std::to_string(vs) + ")");
    return TDTK_EUNSUP;
  }
  return TDTK_OK;
}

}  // namespace

extern "C" {

int tdtk_voxel_walk(int device, const double* starts, const double* ends, size_t m, double voxel_size, uint64_t* offsets,
                    int32_t* voxels, size_t cap, uint64_t* total)
{
  if (!offsets || !total || (m && (!starts || !ends))) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (!(voxel_size > 0) || !std::isfinite(voxel_size)) { set_error("voxel_size must be finite and > 0"); return TDTK_EINVAL; }
  if (m >= 0x7FFFFFFFull) { set_error("too many rays for one call"); return TDTK_EUNSUP; }
  if (!m) { offsets[0] = 0; *total = 0; return TDTK_OK; }
  Ctx* c;
  int rc;
  if ((rc = get_ctx(device, &c, false))) return rc;
  hipStream_t s = c->stream;
  const size_t tmpb = scan_u32_temp_bytes(m + 1);
  const size_t need = 2 * (3 * m * sizeof(double) + 256) + 2 * ((m + 1) * sizeof(uint32_t) + 256) + tmpb + 1024;
  if ((rc = c->ws[WS_ARENA].ensure(need))) return rc;
  Bump b{c->ws[WS_ARENA].as<char>()};
  double* d_s = b.take<double>(3 * m);
  double* d_e = b.take<double>(3 * m);
  uint32_t* d_cnt = b.take<uint32_t>(m + 1);
  uint32_t* d_off = b.take<uint32_t>(m + 1);
  unsigned long long* d_ctr = b.take<unsigned long long>(8);
  void* d_tmp = b.take<char>(tmpb);
  HIPCHK(hipMemcpyAsync(d_s, starts, 3 * m * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_e, ends, 3 * m * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(d_ctr, 0, 8 * sizeof(unsigned long long), s));
  HIPCHK(launch_vox_walk_check(d_s, d_e, m, voxel_size, d_ctr, s));
  unsigned long long h_ctr[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(h_ctr, d_ctr, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if ((rc = vox_input_error(h_ctr[0], voxel_size))) return rc;      // before any walk: a walk converts quotients to integers
  HIPCHK(launch_vox_walk_count(d_s, d_e, m, voxel_size, d_cnt, d_ctr, s));
  HIPCHK(hipMemcpyAsync(h_ctr, d_ctr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (h_ctr[1] > 0xFFFFFFFFull) { set_error("the rays of one call visit more than 2^32 - 1 voxels"); return TDTK_EUNSUP; }
  HIPCHK(launch_scan_u32(d_cnt, d_off, m + 1, d_tmp, tmpb, s));
  std::vector<uint32_t> h_off(m + 1);
  HIPCHK(hipMemcpyAsync(h_off.data(), d_off, (m + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (size_t i = 0; i <= m; ++i) offsets[i] = h_off[i];
  *total = h_ctr[1];
  if (!h_ctr[1]) return TDTK_OK;
  if (cap < h_ctr[1] || !voxels) {
    set_error("cap " + std::to_string(cap) + " < total " + std::to_string(h_ctr[1]));
    return TDTK_EINVAL;
  }
  if ((rc = c->ws[WS_TMPA].ensure(3 * (size_t)h_ctr[1] * sizeof(int32_t)))) return rc;
  HIPCHK(launch_vox_walk_fill(d_s, d_e, m, voxel_size, d_off, c->ws[WS_TMPA].as<int32_t>(), s));
  HIPCHK(hipMemcpyAsync(voxels, c->ws[WS_TMPA].p, 3 * (size_t)h_ctr[1] * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return TDTK_OK;
}

int tdtk_peopleremover(int device, const double* xyz, const uint64_t* scan_offsets, const double* origins, const double* ray_ends,
                       size_t S, double voxel_size, uint64_t diff, uint64_t cluster_size, int subvoxel, uint8_t* dynamic,
                       int32_t* free_voxels, size_t cap, uint64_t* info)
{
  if (!xyz || !scan_offsets || !origins || !dynamic || !info) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (!(voxel_size > 0) || !std::isfinite(voxel_size)) { set_error("voxel_size must be finite and > 0"); return TDTK_EINVAL; }
  if (S == 0) { set_error("no scan"); return TDTK_EINVAL; }
  if (scan_offsets[0] != 0) { set_error("scan_offsets[0] must be 0"); return TDTK_EINVAL; }
  for (size_t i = 0; i < S; ++i)
    if (scan_offsets[i + 1] < scan_offsets[i]) { set_error("scan_offsets must not decrease"); return TDTK_EINVAL; }
  const uint64_t n64 = scan_offsets[S];
  if (n64 == 0) { set_error("no voxel occupied"); return TDTK_EINVAL; }       // peopleremover.cc:200
  if (n64 >= 0x7FFFFFFFull || S >= 0x7FFFFFFFull) { set_error("too many points or scans for one call"); return TDTK_EUNSUP; }
  const size_t n = (size_t)n64;
  Ctx* c;
  int rc;
  if ((rc = get_ctx(device, &c, false))) return rc;
  hipStream_t s = c->stream;
  Events ev;
  if (!ev.ok) { set_error("hipEventCreate failed"); return TDTK_EDEVICE; }

  const size_t tmpb = vox_sort_temp_bytes(n);
  const size_t per_point = 2 * 24 + 2 * 8 + 2 * 4 + 6 * 4 + 4 + 4 + 8 + 8 + 4 + 3;
  const size_t need = n * per_point + S * 28 + tmpb + 40 * 256 + 64 * 8;
  if ((rc = c->ws[WS_ARENA].ensure(need))) return rc;
  Bump b{c->ws[WS_ARENA].as<char>()};
  VoxArgs a{};
  a.n = (uint32_t)n; a.S = (uint32_t)S; a.vs = voxel_size; a.diff = diff; a.subvoxel = subvoxel;
  a.cluster_size = cluster_size > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cluster_size;
  double* d_xyz = b.take<double>(3 * n);
  double* d_ends = ray_ends ? b.take<double>(3 * n) : nullptr;
  double* d_org = b.take<double>(3 * S);
  uint32_t* d_off = b.take<uint32_t>(S + 1);
  a.xyz = d_xyz; a.ends = d_ends; a.origins = d_org; a.scan_off = d_off;
  a.keys = b.take<uint64_t>(n); a.keys_s = b.take<uint64_t>(n);
  a.scans = b.take<uint32_t>(n); a.scans_s = b.take<uint32_t>(n);
  a.fp = b.take<uint32_t>(n + 1); a.fv = b.take<uint32_t>(n + 1); a.fb = b.take<uint32_t>(n + 1);
  a.ip = b.take<uint32_t>(n + 1); a.iv = b.take<uint32_t>(n + 1); a.ib = b.take<uint32_t>(n + 1);
  a.pscan = b.take<uint32_t>(n); a.vstart = b.take<uint32_t>(n + 1);
  a.vkey = b.take<uint64_t>(n); a.bkey = b.take<uint64_t>(n); a.bbase = b.take<uint32_t>(n + 1);
  a.free_mark = b.take<unsigned char>(n); a.pdyn = b.take<unsigned char>(n); a.dynamic = b.take<unsigned char>(n);
  a.parent = a.fp; a.csize = a.fv;          // the head flags are dead once the arrays are compact
  a.ctr = b.take<unsigned long long>(8);
  void* d_tmp = b.take<char>(tmpb);
  if (b.off > c->ws[WS_ARENA].cap) { set_error("internal: voxel workspace undersized"); return TDTK_ENOMEM; }

  std::vector<uint32_t> h_off(S + 1);
  for (size_t i = 0; i <= S; ++i) h_off[i] = (uint32_t)scan_offsets[i];
  HIPCHK(hipEventRecord(ev.e[4], s));
  HIPCHK(hipMemcpyAsync(d_xyz, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, s));
  if (ray_ends) HIPCHK(hipMemcpyAsync(d_ends, ray_ends, 3 * n * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_org, origins, 3 * S * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_off, h_off.data(), (S + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(a.ctr, 0, 8 * sizeof(unsigned long long), s));

  // ---- occupancy ----
  HIPCHK(hipEventRecord(ev.e[0], s));
  HIPCHK(launch_vox_keys(a, s));
  unsigned long long h_ctr[8] = {0};
  HIPCHK(hipMemcpyAsync(h_ctr, a.ctr, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if ((rc = vox_input_error(h_ctr[0], voxel_size))) return rc;
  HIPCHK(launch_vox_sort_flags(a, d_tmp, tmpb, s));
  HIPCHK(launch_vox_compact(a, s));
  uint32_t tot[3] = {0, 0, 0};
  HIPCHK(hipMemcpyAsync(&tot[0], a.ip + n, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&tot[1], a.iv + n, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&tot[2], a.ib + n, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  a.n_pairs = tot[0]; a.n_vox = tot[1]; a.n_bricks = tot[2];
  size_t slots = 64;
  while (slots < 2 * (size_t)a.n_bricks) slots <<= 1;
  if ((rc = c->ws[WS_TMPA].ensure(slots * sizeof(VoxBrick)))) return rc;
  a.table = c->ws[WS_TMPA].as<VoxBrick>();
  a.mask = (uint32_t)(slots - 1);
  HIPCHK(hipMemsetAsync(a.table, 0xFF, slots * sizeof(VoxBrick), s));      // every key VOX_EMPTY
  HIPCHK(launch_vox_table(a, s));
  HIPCHK(hipMemsetAsync(a.free_mark, 0, a.n_vox, s));
  // ---- walk ----
  HIPCHK(hipEventRecord(ev.e[1], s));
  HIPCHK(launch_vox_carve(a, s));
  HIPCHK(hipEventRecord(ev.e[2], s));
  // ---- cluster filter, half-free voxels, classification ----
  HIPCHK(launch_collide_count(a.free_mark, a.n_vox, a.ctr + 2, s));
  if (a.cluster_size > 1u) HIPCHK(launch_vox_cluster_filter(a, s));         // peopleremover.cc:337
  HIPCHK(launch_collide_count(a.free_mark, a.n_vox, a.ctr + 3, s));
  HIPCHK(launch_vox_classify(a, s));
  HIPCHK(hipEventRecord(ev.e[3], s));
  HIPCHK(hipMemcpyAsync(dynamic, a.dynamic, n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h_ctr, a.ctr, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIPCHK(hipEventRecord(ev.e[5], s));
  HIPCHK(hipStreamSynchronize(s));
  info[0] = a.n_vox; info[1] = h_ctr[2]; info[2] = h_ctr[3]; info[3] = h_ctr[4]; info[4] = h_ctr[1];
  float ms = 0.f;
  for (int k = 0; k < 3; ++k) { HIPCHK(hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1])); t_vox_ms[k] = ms; }
  HIPCHK(hipEventElapsedTime(&ms, ev.e[4], ev.e[5]));
  t_vox_ms[3] = ms;

  if (free_voxels) {      // optional and off the hot path: the marks and keys go to the host, which orders them as std::set does
    if (cap < info[2]) {
      set_error("cap " + std::to_string(cap) + " < free voxels " + std::to_string(info[2]));
      return TDTK_EINVAL;
    }
    std::vector<unsigned char> h_free(a.n_vox);
    std::vector<uint64_t> h_key(a.n_vox);
    HIPCHK(hipMemcpyAsync(h_free.data(), a.free_mark, a.n_vox, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_key.data(), a.vkey, (size_t)a.n_vox * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    struct V3 { int32_t x, y, z; };
    std::vector<V3> out;
    out.reserve((size_t)info[2]);
    for (uint32_t v = 0; v < a.n_vox; ++v)
      if (h_free[v]) {
        int64_t x, y, z;
        vox_unkey(h_key[v], x, y, z);
        out.push_back(V3{(int32_t)x, (int32_t)y, (int32_t)z});
      }
    std::sort(out.begin(), out.end(), [](const V3& p, const V3& q) {      // struct voxel's operator<, common.h:51-60
      if (p.x != q.x) return p.x < q.x;
      if (p.y != q.y) return p.y < q.y;
      return p.z < q.z;
    });
    for (size_t i = 0; i < out.size(); ++i) { free_voxels[3 * i] = out[i].x; free_voxels[3 * i + 1] = out[i].y; free_voxels[3 * i + 2] = out[i].z; }
  }
  return TDTK_OK;
}

int tdtk_peopleremover_timings(double* ms4)
{
  if (!ms4) { set_error("NULL argument"); return TDTK_EINVAL; }
  for (int k = 0; k < 4; ++k) ms4[k] = t_vox_ms[k];
  return TDTK_OK;
}

}  // extern "C"
