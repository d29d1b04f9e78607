// The geometry of the reference's four Hough accumulators (src/shapes/accumulator.cc), host only: no HIP header, so that
// hough_host.cpp also builds on its own for the CPU-tier tests.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace tdtk {

struct HoughGeom {
  int type = 0;
  uint32_t rho_num = 0, phi_num = 0, theta_num = 0, rho_max = 0;
  std::vector<int> slices;       // cells per phi slice (types 0, 1, 3); type 2: six faces of nrCells^2
  int nr_cells = 0;              // type 2: ThetaNum / 4
  double phi_top_rad = 0.0, step = 0.0;      // type 3
  size_t cells = 0;
};
// TDTK_OK, or the code with err set: the argument checks of tdtk_hough_normals
int hough_geometry(int type, uint32_t rho_num, uint32_t phi_num, uint32_t theta_num, uint32_t rho_max, HoughGeom& g, std::string& err);
void hough_geom_normals(const HoughGeom& g, double* normals);      // [g.cells][3]
// the reference's getMax(int* cell): entry -> { nx, ny, nz, rho }
void hough_geom_cell_plane(const HoughGeom& g, const int32_t* cell, double plane[4]);
// (count, linear index = cell * rho_num + k) records -> the reference's multiset order and entry layout; entries [n][4 or 5]
void hough_order_peaks(const HoughGeom& g, std::vector<std::pair<int32_t, uint32_t>>& rec, int32_t* entries);
// calcPlane's ending (hough.cc:1283-1309) from the centroid and the six centred moments (linalg.cpp: jacobi_eigen<3>)
void hough_plane_from_moments(const double c[3], const double m[6], double plane[4], double* planarity);

}  // namespace tdtk
