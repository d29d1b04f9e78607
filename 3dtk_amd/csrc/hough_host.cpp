// The geometry of the reference's four Hough accumulators (src/shapes/accumulator.cc, hsm3d.cc), restated as written: which
// normal a cell votes with (the loops of accumulate(Point)), which plane a cell stands for (getMax(int* cell) -- not the same
// formulas), and the order in which getMax() lists the cells.  Host only, no HIP header: tests/test_hough_host.py builds this
// file on its own.  Every expression keeps the reference's order of operations; the library is built without contraction.
#include <algorithm>
#include <cmath>

#include "hough_geom.h"
#include "tdtk_hip.h"

namespace tdtk {

namespace {

// globals.icc:172-187
inline double rad(const double deg) { return (2 * M_PI * deg) / 360; }
inline double deg(const double rad) { return (rad * 360) / (2 * M_PI); }

// globals.icc:253-259
inline void normalize3(double* x)
{
  const double norm = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  x[0] /= norm;
  x[1] /= norm;
  x[2] /= norm;
}

// accumulator.cc:17-24
inline void polar2normal(const double theta, const double phi, double* n)
{
  n[0] = std::cos(theta) * std::sin(phi);
  n[1] = std::sin(theta) * std::sin(phi);
  n[2] = std::cos(phi);
  normalize3(n);
}

// hsm3d.cc:117-168.  A face outside 1 .. 6 leaves the reference's result uninitialised; here it is NaN.
inline void coords_cube_to_s2(const unsigned face, const unsigned i, const unsigned j, const unsigned width, double* result)
{
  double u = (i - 0.5) / (static_cast<double>(width));
  u = u * 2 - 1;
  double v = (j - 0.5) / (static_cast<double>(width));
  v = v * 2 - 1;
  switch (face) {
    case 1: result[0] = 1; result[1] = u; result[2] = v; break;
    case 4: result[0] = -1; result[1] = -u; result[2] = -v; break;
    case 2: result[0] = u; result[1] = 1; result[2] = v; break;
    case 5: result[0] = -u; result[1] = -1; result[2] = -v; break;
    case 3: result[0] = u; result[1] = v; result[2] = 1; break;
    case 6: result[0] = -u; result[1] = -v; result[2] = -1; break;
    default: result[0] = result[1] = result[2] = std::nan(""); break;
  }
  const double norm = std::sqrt(result[0] * result[0] + result[1] * result[1] + result[2] * result[2]);
  result[0] /= norm;
  result[1] /= norm;
  result[2] /= norm;
}

}  // namespace

int hough_geometry(int type, uint32_t rho_num, uint32_t phi_num, uint32_t theta_num, uint32_t rho_max, HoughGeom& g, std::string& err)
{
  g = HoughGeom();
  g.type = type; g.rho_num = rho_num; g.phi_num = phi_num; g.theta_num = theta_num; g.rho_max = rho_max;
  if (type < 0 || type > 3) { err = "accumulator type must be 0 (Simple), 1 (Ball), 2 (Cube) or 3 (BallI)"; return TDTK_EINVAL; }
  if (rho_num < 1 || phi_num < 1 || theta_num < 1) { err = "RhoNum, PhiNum and ThetaNum must be at least 1"; return TDTK_EINVAL; }
  if (phi_num >= (1u << 24) || theta_num >= (1u << 24)) { err = "PhiNum and ThetaNum must stay below 2^24"; return TDTK_EUNSUP; }
  if (type == 0) {
    g.slices.assign(phi_num, (int)theta_num);
  } else if (type == 1) {
    // AccumulatorBall::AccumulatorBall, accumulator.cc:312-354: one slice per trip of a loop over an accumulated double
    if (theta_num < 2) { err = "AccumulatorBall: ThetaNum must be at least 2 (the reference divides by ThetaNum - 1)"; return TDTK_EUNSUP; }
    const double step = 180.0 / phi_num;
    const double MAX_A = 2 * M_PI * 1.0;
    double r = std::sin(rad(0.0));
    size_t counter = 0;
    for (double phi = 0; phi < 180.0; phi += step) {
      if (counter >= phi_num) {
        err = "AccumulatorBall: with PhiNum " + std::to_string(phi_num) + " the reference's constructor runs its slice loop more than "
              "PhiNum times (phi += 180.0 / PhiNum stays below 180.0 after PhiNum additions) and writes outside ballNr; accepted "
              "are the PhiNum for which that loop runs exactly PhiNum times";
        return TDTK_EUNSUP;
      }
      const double r_next = std::sin(rad(phi + step));
      const double a = 2 * M_PI * (r + r_next) / 2.0;
      const double c = ((360.0 * (MAX_A / a)) / (theta_num - 1));
      const double cells = 1.0 + 360.0 / c;
      if (!(cells >= 1.0 && cells < 2147483648.0)) { err = "AccumulatorBall: a slice's size does not fit an int"; return TDTK_EUNSUP; }
      g.slices.push_back((int)cells);
      r = r_next;
      counter++;
    }
    if (counter != phi_num) {
      err = "AccumulatorBall: with PhiNum " + std::to_string(phi_num) + " the reference's slice loop ends early and reads slices it "
            "never sized";
      return TDTK_EUNSUP;
    }
  } else if (type == 2) {
    g.nr_cells = (int)(theta_num / 4);
    if (g.nr_cells < 1) { err = "AccumulatorCube: ThetaNum must be at least 4 (nrCells = ThetaNum / 4)"; return TDTK_EUNSUP; }
    g.slices.assign(6, g.nr_cells * g.nr_cells);
  } else {
    // AccumulatorBallI::AccumulatorBallI, accumulator.cc:1427-1458
    if (phi_num < 3) {
      err = "AccumulatorBallI: PhiNum must be at least 3 (with 1 or 2 the reference's step is negative or infinite)";
      return TDTK_EUNSUP;
    }
    double step = 180.0 / phi_num;
    const double h_0 = std::cos(rad(90 - step));
    const double MAX_A = (2.0 * M_PI * h_0) / theta_num;
    const double h_top = MAX_A / (2.0 * M_PI);
    g.phi_top_rad = std::acos(1 - h_top);
    const double phi_top_deg = deg(g.phi_top_rad);
    step = (180.0 - 2.0 * phi_top_deg) / (double)(phi_num - 2.0);
    g.step = step;
    if (!(step > 0.0) || !(phi_top_deg < 90.0)) { err = "AccumulatorBallI: no slice between the pole cells"; return TDTK_EUNSUP; }
    std::vector<int> nr(phi_num, -1);
    size_t counter = 0;
    nr[counter] = 1;
    nr[phi_num - 1 - counter] = 1;
    counter++;
    for (double phi = phi_top_deg; phi < 90; phi += step) {
      if (counter > phi_num - 1) {
        err = "AccumulatorBallI: the reference's constructor writes outside ballNr for PhiNum " + std::to_string(phi_num) +
              ", ThetaNum " + std::to_string(theta_num);
        return TDTK_EUNSUP;
      }
      const double h_i = std::cos(rad(phi)) - std::cos(rad(phi + step));
      const double a_i = 2 * M_PI * h_i;
      const double cells = a_i / MAX_A;
      if (!(cells >= 0.0 && cells < 2147483648.0)) { err = "AccumulatorBallI: a slice's size does not fit an int"; return TDTK_EUNSUP; }
      nr[counter] = (int)cells;
      nr[phi_num - 1 - counter] = (int)cells;
      counter++;
    }
    for (int v : nr)
      if (v < 0) { err = "AccumulatorBallI: the reference's constructor leaves a slice unsized"; return TDTK_EUNSUP; }
    g.slices = nr;
  }
  g.cells = 0;
  for (int v : g.slices) g.cells += (size_t)v;
  return TDTK_OK;
}

void hough_geom_normals(const HoughGeom& g, double* normals)
{
  double* n = normals;
  if (g.type == 2) {
    // AccumulatorCube::accumulate(Point), accumulator.cc:1252-1262: Normalize3 on the already normalised vector, as written
    for (int i = 0; i < 6; i++)
      for (int j = 1; j <= g.nr_cells; j++)
        for (int k = 1; k <= g.nr_cells; k++) {
          coords_cube_to_s2((unsigned)(i + 1), (unsigned)j, (unsigned)k, (unsigned)g.nr_cells, n);
          normalize3(n);
          n += 3;
        }
    return;
  }
  for (unsigned int i = 0; i < g.phi_num; i++) {
    double phi;
    if (g.type == 0) phi = (i + 0.5) * M_PI / (g.phi_num * 0.99999999999);            // :128
    else if (g.type == 1) phi = (i + 0.5) * M_PI / (g.phi_num * 0.999999999);         // :453
    else phi = g.phi_top_rad + (i - 0.5) * rad(g.step);                              // :1566
    for (int j = 0; j < g.slices[i]; j++) {
      double theta = (j + 0.5) * 2 * M_PI / g.slices[i];                              // :131, :455, :1568
      if (theta > 2 * M_PI) theta = 2 * M_PI;
      if (phi > M_PI) phi = M_PI;
      if (g.type == 3 && i == 0) {
        n[0] = 0.0; n[1] = 0.0; n[2] = 1.0;
      } else if (g.type == 3 && i == g.rho_num - 1) {                                 // :1578, RhoNum as written
        n[0] = 0.0; n[1] = 0.0; n[2] = -1.0;
      } else {
        n[0] = std::cos(theta) * std::sin(phi);
        n[1] = std::sin(theta) * std::sin(phi);
        n[2] = std::cos(phi);
        normalize3(n);
      }
      n += 3;
    }
  }
}

void hough_geom_cell_plane(const HoughGeom& g, const int32_t* cell, double plane[4])
{
  if (g.type == 2) {
    // AccumulatorCube::getMax(int*), accumulator.cc:1355-1371, as written: the face is cell[1] + 1, the patch cell[2], cell[3]
    // and rho comes from cell[0] -- not the layout in which getMax() lists a cell (count, rho, face, i, j)
    const double rho = (cell[0] + 0.5) * (double)g.rho_max / (double)g.rho_num;
    coords_cube_to_s2((unsigned)(unsigned short)(cell[1] + 1), (unsigned)cell[2], (unsigned)cell[3], (unsigned)g.nr_cells, plane);
    plane[3] = rho;
    return;
  }
  const double rho = (cell[1] + 0.5) * (double)g.rho_max / (double)g.rho_num;
  if (g.type == 0) {                                                                  // :255-264
    const double phi = (0.5 + cell[3]) * (double)(M_PI / (double)g.phi_num);
    const double theta = (0.5 + cell[2]) * (double)(2.0 * M_PI / (double)g.theta_num);
    polar2normal(theta, phi, plane);
  } else if (g.type == 1) {                                                           // :574-587
    const double phi = (0.5 + cell[3]) * (double)(M_PI / (double)g.phi_num);
    const int bNr = g.slices[cell[3]];
    const double theta = (0.5 + cell[2]) * (double)(2.0 * M_PI / bNr);
    polar2normal(theta, phi, plane);
  } else {                                                                            // :1700-1727
    if (cell[3] == 0) {
      plane[0] = 0.0; plane[1] = 0.0; plane[2] = 1.0;
    } else if ((unsigned int)cell[3] == g.phi_num - 1) {
      plane[0] = 0.0; plane[1] = 0.0; plane[2] = -1.0;
    } else {
      const double phi = g.phi_top_rad + (-0.5 + cell[3]) * rad(g.step);
      const double bNr = g.slices[cell[3]];
      const double theta = (0.5 + cell[2]) * (double)(2.0 * M_PI / bNr);
      polar2normal(theta, phi, plane);
    }
  }
  plane[3] = rho;
}

void hough_order_peaks(const HoughGeom& g, std::vector<std::pair<int32_t, uint32_t>>& rec, int32_t* entries)
{
  // std::multiset<int*, maxcompare>: count descending, an equal count behind its equals, i.e. in insertion order -- rho, phi,
  // theta for types 0, 1, 3 (:269-279, :592-603, :1733-1742), face, i, j, rho for type 2 (:1376-1389)
  const uint64_t C = g.cells, R = g.rho_num;
  auto rank = [&](uint32_t lin) -> uint64_t {
    const uint64_t c = lin / R, k = lin % R;
    return g.type == 2 ? c * R + k : k * C + c;
  };
  std::sort(rec.begin(), rec.end(), [&](const std::pair<int32_t, uint32_t>& a, const std::pair<int32_t, uint32_t>& b) {
    if (a.first != b.first) return a.first > b.first;
    return rank(a.second) < rank(b.second);
  });
  std::vector<uint64_t> first(g.slices.size() + 1, 0);
  for (size_t s = 0; s < g.slices.size(); ++s) first[s + 1] = first[s] + (uint64_t)g.slices[s];
  for (size_t e = 0; e < rec.size(); ++e) {
    const uint64_t c = rec[e].second / R, k = rec[e].second % R;
    const size_t s = (size_t)(std::upper_bound(first.begin(), first.end(), c) - first.begin()) - 1;      // slice / face of cell c
    const uint64_t in = c - first[s];
    if (g.type == 2) {
      int32_t* o = entries + 5 * e;
      o[0] = rec[e].first; o[1] = (int32_t)k; o[2] = (int32_t)s; o[3] = (int32_t)(in / (uint64_t)g.nr_cells);
      o[4] = (int32_t)(in % (uint64_t)g.nr_cells);
    } else {
      int32_t* o = entries + 4 * e;
      o[0] = rec[e].first; o[1] = (int32_t)k; o[2] = (int32_t)in; o[3] = (int32_t)s;
    }
  }
}

}  // namespace tdtk
