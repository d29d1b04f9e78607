// The Hough-transform entry points: tdtk_hough_normals, _vote, _peaks, _cell_plane, _plane_points, _fit_plane, _timings
// (kernels: hough.hip, per-lane code: hough_lane.h, the accumulators' geometry: hough_host.cpp).
#include "api_internal.h"
#include "hough.h"

using namespace tdtk;

namespace {

struct Events {
  hipEvent_t e[2] = {nullptr, nullptr};
  bool ok = true;
  Events() { for (auto& x : e) if (hipEventCreate(&x) != hipSuccess) { x = nullptr; ok = false; } }
  ~Events() { for (auto& x : e) if (x) (void)hipEventDestroy(x); }
};

thread_local double t_hough_ms[4] = {0.0, 0.0, 0.0, 0.0};
thread_local uint64_t t_hough_allocs = 0;

int ensure(DevBuf& b, size_t bytes)
{
  const size_t before = b.cap;
  const int rc = b.ensure(bytes ? bytes : 8);
  if (b.cap != before) t_hough_allocs += 1;
  return rc;
}

int geometry(int type, const uint32_t* dims, HoughGeom& g)
{
  std::string err;
  const int rc = hough_geometry(type, dims[0], dims[1], dims[2], dims[3], g, err);
  if (rc) set_error(err);
  return rc;
}

// the cloud on the device: uploaded, or the resident one
int cloud(Ctx* c, const double* xyz, size_t N, const double** d_xyz)
{
  if (xyz) {
    int rc;
    c->hough_have_xyz = false;
    if ((rc = ensure(c->hough_xyz, 3 * N * sizeof(double)))) return rc;
    if (N) HIPCHK(hipMemcpyAsync(c->hough_xyz.p, xyz, 3 * N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    c->hough_n = N;
    c->hough_have_xyz = true;
  } else if (!c->hough_have_xyz || c->hough_n != N) {
    set_error("xyz is NULL and this thread has no resident cloud of " + std::to_string(N) + " points on the device");
    return TDTK_EINVAL;
  }
  *d_xyz = c->hough_xyz.as<double>();
  return TDTK_OK;
}

int elapsed(Events& ev, int slot)
{
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  t_hough_ms[slot] = ms;
  return TDTK_OK;
}

}  // namespace

extern "C" {

int tdtk_hough_normals(int type, const uint32_t* dims, double* normals, size_t cap, size_t* C, int32_t* slice_sizes)
{
  if (!dims || !C) { set_error("NULL argument"); return TDTK_EINVAL; }
  HoughGeom g;
  int rc;
  if ((rc = geometry(type, dims, g))) return rc;
  *C = g.cells;
  if (slice_sizes) for (size_t i = 0; i < g.slices.size(); ++i) slice_sizes[i] = g.slices[i];
  if (cap < g.cells || (!normals && g.cells)) {
    if (!normals && cap == 0) return TDTK_OK;      // a count
    set_error("cap " + std::to_string(cap) + " < cells " + std::to_string(g.cells));
    return TDTK_EINVAL;
  }
  hough_geom_normals(g, normals);
  return TDTK_OK;
}

int tdtk_hough_cell_plane(int type, const uint32_t* dims, const int32_t* cell, double* plane4)
{
  if (!dims || !cell || !plane4) { set_error("NULL argument"); return TDTK_EINVAL; }
  HoughGeom g;
  int rc;
  if ((rc = geometry(type, dims, g))) return rc;
  if ((type == 1 || type == 3) && (cell[3] < 0 || (uint32_t)cell[3] >= g.phi_num)) {
    set_error("the cell's phi index lies outside the accumulator");
    return TDTK_EINVAL;
  }
  hough_geom_cell_plane(g, cell, plane4);
  return TDTK_OK;
}

int tdtk_hough_vote(int device, const double* xyz, size_t N, const double* normals, size_t C, uint32_t RhoNum, uint32_t RhoMax,
                    double D, int32_t* counts)
{
  if (!normals) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (N >= 0x80000000ull) { set_error("too many points for one call (N >= 2^31)"); return TDTK_EUNSUP; }
  Ctx* c;
  int rc;
  if ((rc = get_ctx(device, &c, false))) return rc;
  if (!C || !RhoNum) { set_error("C and RhoNum must be at least 1"); return TDTK_EINVAL; }
  if ((unsigned __int128)C * RhoNum >= 0x80000000ull) { set_error("accumulator too large for one call (C * RhoNum >= 2^31)"); return TDTK_EUNSUP; }
  hipStream_t s = c->stream;
  Events ev;
  if (!ev.ok) { set_error("hipEventCreate failed"); return TDTK_EDEVICE; }
  const double* d_xyz = nullptr;
  if ((rc = cloud(c, xyz, N, &d_xyz))) return rc;
  c->hough_have_counts = false;
  const size_t total = C * (size_t)RhoNum;
  if ((rc = ensure(c->hough_normals, 3 * C * sizeof(double)))) return rc;
  if ((rc = ensure(c->hough_counts, total * sizeof(int32_t)))) return rc;
  if ((rc = ensure(c->hough_rho, (size_t)RhoNum * sizeof(double)))) return rc;
  HIPCHK(hipMemcpyAsync(c->hough_normals.p, normals, 3 * C * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipEventRecord(ev.e[0], s));
  HIPCHK(launch_hough_vote(d_xyz, (uint32_t)N, c->hough_normals.as<double>(), (uint32_t)C, RhoNum, RhoMax, D, c->hough_rho.as<double>(),
                           c->hough_counts.as<int32_t>(), s));
  HIPCHK(hipEventRecord(ev.e[1], s));
  if (counts) HIPCHK(hipMemcpyAsync(counts, c->hough_counts.p, total * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  c->hough_cells = C; c->hough_rho_num = RhoNum; c->hough_have_counts = true;
  return elapsed(ev, 0);
}

int tdtk_hough_peaks(int device, const int32_t* counts, int type, const uint32_t* dims, double PlaneRatio, int32_t* cells,
                     size_t cap, uint64_t* n, int32_t* max)
{
  if (!dims || !n || !max) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (PlaneRatio != PlaneRatio) { set_error("PlaneRatio is NaN"); return TDTK_EINVAL; }
  Ctx* c;
  int rc;
  if ((rc = get_ctx(device, &c, false))) return rc;
  HoughGeom g;
  if ((rc = geometry(type, dims, g))) return rc;
  if ((unsigned __int128)g.cells * g.rho_num >= 0x80000000ull) { set_error("accumulator too large for one call (C * RhoNum >= 2^31)"); return TDTK_EUNSUP; }
  const size_t total = g.cells * (size_t)g.rho_num;
  if (!counts && (!c->hough_have_counts || c->hough_cells != g.cells || c->hough_rho_num != g.rho_num)) {
    set_error("counts is NULL and this thread's last vote on the device is not of this accumulator");
    return TDTK_EINVAL;
  }
  hipStream_t s = c->stream;
  Events ev;
  if (!ev.ok) { set_error("hipEventCreate failed"); return TDTK_EDEVICE; }
  if (counts) {
    c->hough_have_counts = false;
    if ((rc = ensure(c->hough_counts, total * sizeof(int32_t)))) return rc;
    if (total) HIPCHK(hipMemcpyAsync(c->hough_counts.p, counts, total * sizeof(int32_t), hipMemcpyHostToDevice, s));
    c->hough_cells = g.cells; c->hough_rho_num = g.rho_num; c->hough_have_counts = true;
  }
  const int32_t* d_counts = c->hough_counts.as<int32_t>();
  if ((rc = c->ws[WS_CNT].ensure(256))) return rc;
  int32_t* d_max = c->ws[WS_CNT].as<int32_t>();
  uint32_t* d_n = c->ws[WS_CNT].as<uint32_t>() + 1;
  HIPCHK(hipMemsetAsync(d_max, 0, 8, s));
  HIPCHK(hipEventRecord(ev.e[0], s));
  HIPCHK(launch_hough_max(d_counts, total, d_max, s));
  int32_t h_max = 0;
  HIPCHK(hipMemcpyAsync(&h_max, d_max, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  // hough.cc:248-253: tmpMax = max * PlaneRatio (a double); the loop goes on while (*it)[0] > (int)tmpMax.  A product outside
  // int's range has no defined conversion in the reference; here it saturates.
  const double tm = (double)h_max * PlaneRatio;
  const int32_t threshold = tm >= 2147483647.0 ? 2147483647 : (tm <= -2147483648.0 ? (-2147483647 - 1) : (int32_t)tm);
  HIPCHK(launch_hough_peaks(d_counts, total, threshold, nullptr, 0, d_n, s));
  uint32_t h_n = 0;
  HIPCHK(hipMemcpyAsync(&h_n, d_n, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *n = h_n;
  *max = h_max;
  if (!h_n) { HIPCHK(hipEventRecord(ev.e[1], s)); HIPCHK(hipStreamSynchronize(s)); return elapsed(ev, 1); }
  if (cap < h_n || !cells) {
    set_error("cap " + std::to_string(cap) + " < peaks " + std::to_string(h_n));
    return TDTK_EINVAL;
  }
  if ((rc = c->ws[WS_TMPA].ensure(2 * (size_t)h_n * sizeof(int32_t)))) return rc;
  HIPCHK(hipMemsetAsync(d_n, 0, 4, s));
  HIPCHK(launch_hough_peaks(d_counts, total, threshold, c->ws[WS_TMPA].as<int32_t>(), h_n, d_n, s));
  std::vector<int32_t> raw(2 * (size_t)h_n);
  HIPCHK(hipMemcpyAsync(raw.data(), c->ws[WS_TMPA].p, raw.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipEventRecord(ev.e[1], s));
  HIPCHK(hipStreamSynchronize(s));
  std::vector<std::pair<int32_t, uint32_t>> rec(h_n);
  for (size_t i = 0; i < h_n; ++i) rec[i] = {raw[2 * i], (uint32_t)raw[2 * i + 1]};
  hough_order_peaks(g, rec, cells);
  return elapsed(ev, 1);
}

int tdtk_hough_plane_points(int device, const double* xyz, size_t N, const double* n, double rho, double D, uint8_t* mask,
                            int32_t* indices, size_t cap, uint64_t* count)
{
  if (!n || !count) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (N >= 0x80000000ull) { set_error("too many points for one call (N >= 2^31)"); return TDTK_EUNSUP; }
  Ctx* c;
  int rc;
  if ((rc = get_ctx(device, &c, false))) return rc;
  hipStream_t s = c->stream;
  Events ev;
  if (!ev.ok) { set_error("hipEventCreate failed"); return TDTK_EDEVICE; }
  const double* d_xyz = nullptr;
  if ((rc = cloud(c, xyz, N, &d_xyz))) return rc;
  // Normalize3 (globals.icc:253-259), hough.cc:761
  double nn[3] = {n[0], n[1], n[2]};
  const double norm = std::sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
  nn[0] /= norm; nn[1] /= norm; nn[2] /= norm;
  const size_t tmpb = scan_u32_temp_bytes(N + 1);
  const size_t a256 = 255;
  const size_t o_flags = 0, o_offs = o_flags + (((N + 1) * 4 + a256) & ~a256), o_mask = o_offs + (((N + 1) * 4 + a256) & ~a256),
               o_tmp = o_mask + ((N + a256 + 1) & ~a256), need = o_tmp + tmpb + 256;
  if ((rc = c->ws[WS_ARENA].ensure(need))) return rc;
  char* base = c->ws[WS_ARENA].as<char>();
  uint32_t* d_flags = reinterpret_cast<uint32_t*>(base + o_flags);
  uint32_t* d_offs = reinterpret_cast<uint32_t*>(base + o_offs);
  uint8_t* d_mask = reinterpret_cast<uint8_t*>(base + o_mask);
  HIPCHK(hipEventRecord(ev.e[0], s));
  HIPCHK(launch_hough_plane_mask(d_xyz, (uint32_t)N, nn, rho, D, d_mask, d_flags, s));
  HIPCHK(launch_scan_u32(d_flags, d_offs, N + 1, base + o_tmp, tmpb, s));
  uint32_t h_count = 0;
  HIPCHK(hipMemcpyAsync(&h_count, d_offs + N, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if (mask && N) HIPCHK(hipMemcpyAsync(mask, d_mask, N, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *count = h_count;
  const bool fill = h_count && cap >= h_count && indices;
  if (fill) {
    if ((rc = c->ws[WS_TMPA].ensure((size_t)h_count * sizeof(int32_t)))) return rc;
    HIPCHK(launch_hough_plane_fill(d_flags, d_offs, (uint32_t)N, c->ws[WS_TMPA].as<int32_t>(), s));
    HIPCHK(hipMemcpyAsync(indices, c->ws[WS_TMPA].p, (size_t)h_count * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipEventRecord(ev.e[1], s));
  HIPCHK(hipStreamSynchronize(s));
  if ((rc = elapsed(ev, 2))) return rc;
  if (h_count && !fill && !(mask && !indices && cap == 0)) {
    set_error("cap " + std::to_string(cap) + " < plane points " + std::to_string(h_count));
    return TDTK_EINVAL;
  }
  return TDTK_OK;
}

int tdtk_hough_fit_plane(int device, const double* xyz, size_t N, const int32_t* indices, size_t m, double* plane4, double* planarity)
{
  if (!plane4 || !planarity || (m && !indices)) { set_error("NULL argument"); return TDTK_EINVAL; }
  if (N >= 0x80000000ull) { set_error("too many points for one call (N >= 2^31)"); return TDTK_EUNSUP; }
  for (size_t i = 0; i < m; ++i)
    if (indices[i] < 0 || (size_t)indices[i] >= N) { set_error("index " + std::to_string(indices[i]) + " outside the cloud"); return TDTK_EINVAL; }
  if (m >= 0x80000000ull) { set_error("too many indices for one call (m >= 2^31)"); return TDTK_EUNSUP; }
  Ctx* c;
  int rc;
  if ((rc = get_ctx(device, &c, false))) return rc;
  hipStream_t s = c->stream;
  const double* d_xyz = nullptr;
  if ((rc = cloud(c, xyz, N, &d_xyz))) return rc;
  if (m < 3) { *planarity = 0.0; return TDTK_OK; }      // hough.cc:1257
  Events ev;
  if (!ev.ok) { set_error("hipEventCreate failed"); return TDTK_EDEVICE; }
  if ((rc = c->ws[WS_TMPA].ensure(m * sizeof(int32_t)))) return rc;
  if ((rc = c->ws[WS_TMPB].ensure(6 * HOUGH_MOMENT_BLOCKS * sizeof(double)))) return rc;
  int32_t* d_idx = c->ws[WS_TMPA].as<int32_t>();
  double* d_part = c->ws[WS_TMPB].as<double>();
  std::vector<double> part(6 * HOUGH_MOMENT_BLOCKS);
  double cen[3] = {0.0, 0.0, 0.0}, mom[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  HIPCHK(hipMemcpyAsync(d_idx, indices, m * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIPCHK(hipEventRecord(ev.e[0], s));
  HIPCHK(launch_hough_moments(d_xyz, d_idx, (uint32_t)m, 0, cen, d_part, s));
  HIPCHK(hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (uint32_t b = 0; b < HOUGH_MOMENT_BLOCKS; ++b) for (int q = 0; q < 3; ++q) cen[q] += part[6 * b + q];
  const int n_int = (int)m;
  for (int q = 0; q < 3; ++q) cen[q] /= n_int;      // hough.cc:1269-1271
  HIPCHK(launch_hough_moments(d_xyz, d_idx, (uint32_t)m, 1, cen, d_part, s));
  HIPCHK(hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipEventRecord(ev.e[1], s));
  HIPCHK(hipStreamSynchronize(s));
  for (uint32_t b = 0; b < HOUGH_MOMENT_BLOCKS; ++b) for (int q = 0; q < 6; ++q) mom[q] += part[6 * b + q];
  hough_plane_from_moments(cen, mom, plane4, planarity);
  return elapsed(ev, 3);
}

int tdtk_hough_timings(double* ms5)
{
  if (!ms5) { set_error("NULL argument"); return TDTK_EINVAL; }
  for (int k = 0; k < 4; ++k) ms5[k] = t_hough_ms[k];
  ms5[4] = (double)t_hough_allocs;
  return TDTK_OK;
}

}  // extern "C"
