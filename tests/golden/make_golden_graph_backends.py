"""Generator of k16_graph_backends.npz: the four graph-SLAM back-ends -- lum6DEuler (-G 1, lum6Deuler.cc), lum6DQuat (-G 2,
lum6Dquat.cc), ghelix6DQ2 (-G 3, ghelix6DQ2.cc) and gapx6D (-G 4, gapx6D.cc) -- from the reference's own compiled sources:
the per-link quantities of their member functions and whole doGraphSlam6D calls with nrIt 1 and 2, on the link cases and
graphs of tests/graph_backend_cases.py (the fixture stores results; the clouds come from seeds).

    python tests/golden/make_golden_graph_backends.py        (needs the reference checkout: $TDTK_REF, default /root/reference)

lum6Deuler.cc, lum6Dquat.cc, ghelix6DQ2.cc, gapx6D.cc, graphSlam6D.cc, graph.cc, icp6Dhelix.cc, icp6Dapx.cc (computeRt),
kdIndexed.cc and the vendored newmat are compiled where they lie, next to a driver of our own (DRIVER below), into a
temporary directory and loaded through ctypes; nothing of them reaches the repository.  The flags are those of
oracle/build_ref.sh with one change, -DOPENMP_NUM_THREADS=1, and the driver calls omp_set_num_threads(1): the reference's
loops over the links add into one matrix from several threads (lum6Dquat.cc:249-275 without a critical section, the others
inside one but in the order the threads arrive), so only the serial order -- link order, which is what the library
implements -- has one result.  With rnd = 1 no value of rand() enters (searchTree.cc:55), so none is recorded.

What stands in for what cannot be built without Boost, CSparse and the scan-IO layer, all of it our own text, none of it
part of what is tested:
  * slam6d/scan.h (SCAN_H) and the bodies in the driver: a Scan that holds a pose and a point set.  The real one drags in
    Boost and the scan-IO layer.  Its constructor follows basicScan.cc:184-192 and :735 (transMat from the pose, points moved
    into the world, dalignxf = identity), transform / transformToEuler / transformToQuat apply the reference's own
    globals.icc functions (compiled here, not copied) in the order of scan.cc:878-898, :1061-1083 and :1093-1104.
    Scan::getPtPairs does what scan.cc:1220-1260 and searchTree.cc:31-90 do for rnd <= 1, in our own words: it asks the
    reference's own KDtreeIndexed (kdIndexed.cc, compiled alongside) once per point, through its own M4inv / transform3,
    and takes the centroids as means over the finished list in list order (the same additions in the same order); `sum`,
    which no back-end reads, is not computed.  The pair search itself is pinned elsewhere (test_oracle_vs_ref.py), and
    the fixture holds a SHA-256 of every link case's pair list so that the tests know they evaluate the same pairs.
  * boost/graph/adjacency_list.hpp (BOOST_H): empty tags and templates; graph.h names them in one typedef nothing uses.
  * cs.h (CS_H) and the eight cs_* functions graphSlam6D.cc calls, in the driver: triplets into a dense matrix, and a dense
    Cholesky solve that reads the upper triangle only, as CSparse does for a symmetric input.  CSparse's own factorisation
    stays unpinned at this one boundary.  The drop rule (|v| > 0.00001) and the triplet fill of graphSlam6D.cc are compiled
    as they are.  cs_cholsol records what it was handed and what it returned: that is how the assembled matrix, the right
    hand side and X of every iteration get out of doGraphSlam6D.
  * the icp6D constructor (icp6D.cc needs the whole scan layer): it stores its arguments; match() is never called.
The driver is compiled with -fno-access-control to reach the private genBBdForLinkedPair / genBArot- / genBAtransForLinkedPair.

lum6DQuat on a graph with a link of fewer than 3 pairs is not run: covarianceQuat leaves the caller's `Matrix Cab` 0 x 0
there (lum6Dquat.cc:217-230) and FillGB3D's `+= CDab` throws out of an OpenMP region, which ends the process.  The fixture
records status -1 for it; the library hands out a zero block and goes on (a deliberate departure).

Per link case <c>:     link_<c>_n, link_<c>_sha (pair list), link_<c>_b<k> (what Ref.link returns: see LINK_LAYOUT)
Per graph <g>, back-end k:  graph_<g>_b<k>_status; _it<j>_A / _rhs / _X / _ok (what cs_cholsol saw in iteration j of the
nrIt = 2 call; A after the drop rule, both triangles), _blocks_it<j> / _npairs_it<j> (the per-link quantities on the scans
as iteration j finds them), _ret<n> and _poses<n> (return value and [scan][transMat 16 | dalignxf 16 | rPos 3 | rPosTheta 3
| rPosQuat 4] after the call with nrIt = n).

Also imported by the tests (Ref, load, LINK_LAYOUT ...), so that the fixture and the live reference are checked the same way."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
import graph_backend_cases as gc  # noqa: E402

OUT = os.path.join(_HERE, "k16_graph_backends.npz")
REF = os.environ.get("TDTK_REF", "/root/reference")
MAX_BYTES = 500 * 1000

# the flags of oracle/build_ref.sh, one thread (see the docstring)
FLAGS = "-std=c++17 -O3 -fPIC -fopenmp -DOPENMP -DOPENMP_NUM_THREADS=1 -DMAX_OPENMP_NUM_THREADS=512 -w".split()
SOURCES = ("lum6Deuler", "lum6Dquat", "ghelix6DQ2", "gapx6D", "graphSlam6D", "graph", "icp6Dhelix", "icp6Dapx", "kdIndexed")
NEWMAT = ("newmat1 newmat2 newmat3 newmat4 newmat5 newmat6 newmat7 newmat8 newmatex bandmat submat myexcept cholesky evalue "
          "fft hholder jacobi newfft sort svd newmatrm newmat9").split()

# what Ref.link returns per back-end: name -> slice
LINK_LAYOUT = {
    1: {"C": slice(0, 36), "CD": slice(36, 42)},
    2: {"C": slice(0, 49), "CD": slice(49, 56)},
    3: {"Blk": slice(0, 36), "bd1": slice(36, 42), "bd2": slice(42, 48), "ret": slice(48, 49)},
    4: {"cm": slice(0, 3), "cd": slice(3, 6), "MkMkt": slice(6, 15), "DkDkt": slice(15, 24), "MkDkt": slice(24, 33),
        "DkMkt": slice(33, 42), "Ak1": slice(42, 45), "Ak2": slice(45, 48), "transA": slice(48, 54), "transBt": slice(54, 57)},
}
LINK_WIDTH = {1: 42, 2: 56, 3: 49, 4: 57}
TRANS_X = np.array([0.01, -0.02, 0.03, -0.015, 0.005, 0.02])     # the X genBAtransForLinkedPair is given in the link cases
POSE_WIDTH = 42

SCAN_H = r"""
#pragma once
// stand-in for include/slam6d/scan.h: a pose and a point set, and only what the graph back-ends touch
#include <string>
#include <vector>
#include "slam6d/ptpair.h"
#include "slam6d/pairingMode.h"
enum nns_type { simpleKD, ANNTree, BOCTree, BruteForce };
class KDtreeIndexed;
class Scan {
public:
  enum AlgoType { INVALID, ICP, ICPINACTIVE, LUM, ELCH };
  static std::vector<Scan*> allScans;
  unsigned int scanNr;
  Scan(const double* xyz, int n, const double* rP, const double* rPT, unsigned int nr);
  ~Scan();
  const double* get_rPos() const { return rPos; }
  const double* get_rPosTheta() const { return rPosTheta; }
  const double* get_rPosQuat() const { return rQuat; }
  const double* get_transMat() const { return transMat; }
  void transformMatrix(const double alignxf[16]);
  void transform(const double alignxf[16], const AlgoType type, int islum = 0);
  void transformToEuler(double rP[3], double rPT[3], const AlgoType type, int islum = 0);
  void transformToQuat(double rP[3], double rPQ[4], const AlgoType type, int islum = 0);
  static void getPtPairs(std::vector<PtPair>* pairs, Scan* Source, Scan* Target, int thread_num, int rnd,
                         double max_dist_match2, double& sum, double* centroid_m, double* centroid_d,
                         PairingMode pairing_mode = CLOSEST_POINT);
  double rPos[3], rPosTheta[3], rQuat[4], transMat[16], dalignxf[16];
  std::vector<double> orig, cur;      // the points the tree holds (world, as loaded) and the current ones
  std::vector<double*> ptrs;
  KDtreeIndexed* kd;
};
"""

BOOST_H = r"""
#pragma once
// stand-in for boost/graph/adjacency_list.hpp: graph.h names these in one typedef that nothing uses
namespace boost {
struct listS {}; struct vecS {}; struct undirectedS {}; struct no_property {};
enum edge_weight_t { edge_weight };
template <class Tag, class T, class Base = no_property> struct property {};
template <class... A> struct adjacency_list {};
}
"""

CS_H = r"""
#pragma once
// stand-in for CSparse's cs.h: triplets into a dense matrix, a dense Cholesky solve over its upper triangle
#include <vector>
struct cs {
  int n;
  std::vector<int> ti, tj;
  std::vector<double> tx, dense;
};
cs* cs_spalloc(int m, int n, int nzmax, int values, int triplet);
int cs_entry(cs* T, int i, int j, double x);
cs* cs_compress(const cs* T);
int cs_dropzeros(cs* A);
int cs_cholsol(int order, const cs* A, double* b);
int cs_qrsol(int order, const cs* A, double* b);
cs* cs_spfree(cs* A);
int cs_print(const cs* A, int brief);
"""

DRIVER = r"""
#include <cmath>
#include <cstring>
#include <iostream>
#include <limits>
#include <sstream>
#include <vector>
#include <omp.h>
#include "slam6d/lum6Deuler.h"
#include "slam6d/lum6Dquat.h"
#include "slam6d/ghelix6DQ2.h"
#include "slam6d/gapx6D.h"
#include "slam6d/kdIndexed.h"
#include "slam6d/globals.icc"

// ---- the stand-in Scan ------------------------------------------------------------------------------------------------
std::vector<Scan*> Scan::allScans;

Scan::Scan(const double* xyz, int n, const double* rP, const double* rPT, unsigned int nr)
{
  scanNr = nr;
  for (int k = 0; k < 3; k++) { rPos[k] = rP[k]; rPosTheta[k] = rPT[k]; }
  double org[16];
  EulerToMatrix4(rPos, rPosTheta, org);                 // basicScan.cc:184
  M4identity(transMat);
  M4identity(dalignxf);
  transformMatrix(org);                                 // :188
  M4identity(dalignxf);                                 // :192
  cur.assign(xyz, xyz + 3 * (size_t)n);
  for (int i = 0; i < n; i++) transform3(org, &cur[3 * (size_t)i]);      // :735
  orig = cur;                                           // copyReducedToOriginal
  ptrs.resize(n);
  for (int i = 0; i < n; i++) ptrs[i] = &orig[3 * (size_t)i];
  kd = new KDtreeIndexed(ptrs.data(), (size_t)n, 20);
}

Scan::~Scan() { delete kd; }

void Scan::transformMatrix(const double alignxf[16])
{
  // what the real Scan does to its matrices on a transform: alignxf goes onto transMat and onto dalignxf from the left,
  // and the Euler and quaternion forms of the pose are read back from the new transMat
  double pose[16], delta[16];
  MMult(alignxf, transMat, pose);
  MMult(alignxf, dalignxf, delta);
  for (int k = 0; k < 16; k++) { transMat[k] = pose[k]; dalignxf[k] = delta[k]; }
  Matrix4ToEuler(transMat, rPosTheta, rPos);
  Matrix4ToQuat(transMat, rQuat);
}

void Scan::transform(const double alignxf[16], const AlgoType, int)     // scan.cc:851-875 (points), then the matrices
{
  for (size_t i = 0; i < cur.size() / 3; i++) transform3(alignxf, &cur[3 * i]);
  transformMatrix(alignxf);
}

// The real Scan reaches a given pose in two moves, not one: first by the inverse of its transMat, then by the pose's own
// matrix.  Points and matrices round twice that way, so the stand-in does the same.
static void set_pose(Scan* s, const double pose[16], Scan::AlgoType type, int islum)
{
  double undo[16];
  M4inv(s->transMat, undo);
  s->transform(undo, Scan::INVALID);
  s->transform(pose, type, islum);
}

void Scan::transformToEuler(double rP[3], double rPT[3], const AlgoType type, int islum)
{
  double pose[16];
  EulerToMatrix4(rP, rPT, pose);
  set_pose(this, pose, type, islum);
}

void Scan::transformToQuat(double rP[3], double rPQ[4], const AlgoType type, int islum)
{
  double pose[16];
  QuatToMatrix4(rPQ, rP, pose);
  set_pose(this, pose, type, islum);
}

void Scan::getPtPairs(std::vector<PtPair>* pairs, Scan* Source, Scan* Target, int thread_num, int rnd,
                      double max_dist_match2, double& sum, double* centroid_m, double* centroid_d, PairingMode)
{
  // every current point of Target asks Source's tree once (rnd <= 1 only, so no draw of rand()).  The tree holds Source's
  // points as loaded: a query goes back through Source's dalignxf, and the point found comes forward through it again.
  // `sum` is a dummy for all four back-ends and is left as it came.
  (void)sum;
  const size_t none = std::numeric_limits<size_t>::max();
  double back[16];
  M4inv(Source->dalignxf, back);
  for (size_t i = 0; 3 * i < Target->cur.size(); i++) {
    double* data = &Target->cur[3 * i];
    double asked[3], model[3];
    transform3(back, data, asked);
    const size_t hit = Source->kd->FindClosest(asked, max_dist_match2, thread_num);
    if (hit == none) continue;
    transform3(Source->dalignxf, &Source->orig[3 * hit], model);
    pairs->push_back(PtPair(model, data));
  }
  // the centroids: means over the finished list, summed in list order; zero for an empty list
  const size_t np = pairs->size();
  double m[3] = { 0, 0, 0 }, d[3] = { 0, 0, 0 };
  for (size_t i = 0; i < np; i++) {
    const PtPair& p = (*pairs)[i];
    m[0] += p.p1.x; m[1] += p.p1.y; m[2] += p.p1.z;
    d[0] += p.p2.x; d[1] += p.p2.y; d[2] += p.p2.z;
  }
  for (int k = 0; k < 3; k++) { centroid_m[k] = np ? m[k] / np : 0.0; centroid_d[k] = np ? d[k] / np : 0.0; }
}

// ---- the stand-in icp6D: stores its arguments -------------------------------------------------------------------------
icp6D::icp6D(icp6Dminimizer* m, double max_dist_match, int max_num_iterations, bool quiet, bool meta, int rnd, bool eP, int anim,
             double epsilonICP, int nns_method, bool cuda_enabled, bool cad_matching, int max_num_metascans)
{
  this->my_icp6Dminimizer = m; this->anim = anim; this->cuda_enabled = cuda_enabled; this->nns_method = nns_method;
  this->max_dist_match2 = max_dist_match * max_dist_match; this->max_num_iterations = max_num_iterations;
  this->quiet = quiet; this->meta = meta; this->rnd = rnd; this->eP = eP; this->epsilonICP = epsilonICP;
  this->cad_matching = cad_matching; this->max_num_metascans = max_num_metascans; this->max_scn_size = 0;
  this->cad_index = 0; this->nr_pointPair = 0;
}
int icp6D::match(Scan*, Scan*, PairingMode) { return 0; }

// ---- the stand-in CSparse ---------------------------------------------------------------------------------------------
struct Rec { int n, ok; std::vector<double> A, b, x; };
static std::vector<Rec> g_rec;

cs* cs_spalloc(int, int, int, int, int) { cs* T = new cs; T->n = 0; return T; }
int cs_entry(cs* T, int i, int j, double x)
{
  T->ti.push_back(i); T->tj.push_back(j); T->tx.push_back(x);
  if (i + 1 > T->n) T->n = i + 1;
  if (j + 1 > T->n) T->n = j + 1;
  return 1;
}
cs* cs_compress(const cs* T)
{
  cs* A = new cs;
  A->n = T->n;
  A->dense.assign((size_t)T->n * T->n, 0.0);
  for (size_t k = 0; k < T->tx.size(); k++) A->dense[(size_t)T->ti[k] * T->n + T->tj[k]] += T->tx[k];     // duplicates add up
  return A;
}
int cs_dropzeros(cs*) { return 1; }
cs* cs_spfree(cs* A) { delete A; return 0; }
int cs_print(const cs*, int) { return 1; }
int cs_qrsol(int, const cs*, double*) { return 0; }
int cs_cholsol(int, const cs* A, double* b)
{
  const int n = A->n;
  Rec r; r.n = n; r.A = A->dense; r.b.assign(b, b + n);
  std::vector<double> L((size_t)n * n, 0.0);
  int ok = 1;
  for (int j = 0; j < n && ok; j++) {               // A = L L^T from the upper triangle: L[i][j] needs A[j][i], j <= i
    double d = A->dense[(size_t)j * n + j];
    for (int k = 0; k < j; k++) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
    if (!(d > 0.0)) { ok = 0; break; }
    d = std::sqrt(d);
    L[(size_t)j * n + j] = d;
    for (int i = j + 1; i < n; i++) {
      double v = A->dense[(size_t)j * n + i];
      for (int k = 0; k < j; k++) v -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
      L[(size_t)i * n + j] = v / d;
    }
  }
  if (ok) {
    for (int i = 0; i < n; i++) {
      double v = b[i];
      for (int k = 0; k < i; k++) v -= L[(size_t)i * n + k] * b[k];
      b[i] = v / L[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; i--) {
      double v = b[i];
      for (int k = i + 1; k < n; k++) v -= L[(size_t)k * n + i] * b[k];
      b[i] = v / L[(size_t)i * n + i];
    }
  }
  r.ok = ok; r.x.assign(b, b + n);
  g_rec.push_back(r);
  return ok;
}

// ---- what the generator calls -----------------------------------------------------------------------------------------
struct Quiet {              // the back-ends narrate on cout / cerr
  std::ostringstream sink;
  std::streambuf *o, *e;
  Quiet() { o = std::cout.rdbuf(sink.rdbuf()); e = std::cerr.rdbuf(sink.rdbuf()); }
  ~Quiet() { std::cout.rdbuf(o); std::cerr.rdbuf(e); }
};

template <class T> static T* make(double maxd)
{
  // (minimizer, mdm, max_dist_match, max_num_iterations, quiet, meta, rnd, eP, anim, epsilonICP, nns_method, epsilonLUM):
  // rnd 1, epsilonLUM < 0 so that every iteration asked for runs
  return new T(0, maxd, maxd, 50, true, false, 1, true, -1, 0.0000001, simpleKD, -1.0);
}

extern "C" {

void* gb_scan_new(const double* xyz, int n, const double* rP, const double* rPT, unsigned int nr) { return new Scan(xyz, n, rP, rPT, nr); }
void gb_scan_free(void* s) { delete (Scan*)s; }
void gb_scan_pose(void* h, double* out)       // transMat 16 | dalignxf 16 | rPos 3 | rPosTheta 3 | rPosQuat 4
{
  Scan* s = (Scan*)h;
  memcpy(out, s->transMat, 16 * sizeof(double)); memcpy(out + 16, s->dalignxf, 16 * sizeof(double));
  memcpy(out + 32, s->get_rPos(), 3 * sizeof(double)); memcpy(out + 35, s->get_rPosTheta(), 3 * sizeof(double));
  memcpy(out + 38, s->get_rPosQuat(), 4 * sizeof(double));
}

// the pair list of a link; p1 / p2 [cap][3] nullable.  Returns the number of pairs.
long gb_pairs(void* first, void* second, double maxd2, long cap, double* p1, double* p2)
{
  omp_set_num_threads(1);
  std::vector<PtPair> uk;
  double sum = 0, cm[3], cd[3];
  Scan::getPtPairs(&uk, (Scan*)first, (Scan*)second, 0, 1, maxd2, sum, cm, cd);
  for (long i = 0; i < (long)uk.size() && i < cap; i++) {
    if (p1) { p1[3 * i] = uk[i].p1.x; p1[3 * i + 1] = uk[i].p1.y; p1[3 * i + 2] = uk[i].p1.z; }
    if (p2) { p2[3 * i] = uk[i].p2.x; p2[3 * i + 1] = uk[i].p2.y; p2[3 * i + 2] = uk[i].p2.z; }
  }
  return (long)uk.size();
}

// the per-link quantities of back-end `backend` from the reference's own member functions; out: LINK_LAYOUT.  X6: the X
// genBAtransForLinkedPair is given (back-end 4).  Returns the number of pairs, -1 on an exception.
long gb_link(int backend, void* first, void* second, double maxd, const double* X6, double* out)
{
  omp_set_num_threads(1);
  Quiet q;
  Scan* a = (Scan*)first; Scan* b = (Scan*)second;
  const double maxd2 = maxd * maxd;
  try {
    std::vector<PtPair> uk;
    double sum = 0, cm[3], cd[3];
    Scan::getPtPairs(&uk, a, b, 0, 1, maxd2, sum, cm, cd);
    const long n = (long)uk.size();
    if (backend == 1) {
      Matrix Cm(6, 6); ColumnVector CD(6);                      // as FillGB3D declares them (lum6Deuler.cc:279-280)
      lum6DEuler::covarianceEuler(a, b, simpleKD, 1, maxd2, &Cm, &CD);
      for (int i = 0; i < 6; i++) { for (int j = 0; j < 6; j++) out[i * 6 + j] = Cm.element(i, j); out[36 + i] = CD.element(i); }
    } else if (backend == 2) {
      Matrix Cm; ColumnVector CD;                               // as FillGB3D declares them (lum6Dquat.cc:258-259)
      lum6DQuat::covarianceQuat(a, b, simpleKD, 1, maxd2, &Cm, &CD);
      for (int i = 0; i < 56; i++) out[i] = 0.0;
      if (Cm.Nrows() == 7)
        for (int i = 0; i < 7; i++) { for (int j = 0; j < 7; j++) out[i * 7 + j] = Cm.element(i, j); out[49 + i] = CD.element(i); }
    } else if (backend == 3) {
      ghelix6DQ2* g = make<ghelix6DQ2>(maxd);
      Matrix B(12, 12); ColumnVector Bd(12); B = 0.0; Bd = 0.0;
      double ret = g->genBBdForLinkedPair(1, 2, &uk, &B, &Bd);  // scans 1 and 2 of three: every block of the link shows
      for (int i = 0; i < 6; i++) {
        for (int j = 0; j < 6; j++) out[i * 6 + j] = B.element(i, j);
        out[36 + i] = Bd.element(i); out[42 + i] = Bd.element(6 + i);
      }
      out[48] = ret;
      delete g;
    } else {
      gapx6D* g = make<gapx6D>(maxd);
      Matrix B(6, 6); ColumnVector A(6); B = 0.0; A = 0.0;
      g->genBArotForLinkedPair(1, 2, &uk, cm, cd, &B, &A);
      for (int k = 0; k < 3; k++) { out[k] = cm[k]; out[3 + k] = cd[k]; out[42 + k] = A.element(k); out[45 + k] = A.element(3 + k); }
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
          out[6 + i * 3 + j] = B.element(i, j);            // MkMkt
          out[15 + i * 3 + j] = B.element(3 + i, 3 + j);   // DkDkt
          out[24 + i * 3 + j] = B.element(3 + i, j);       // MkDkt
          out[33 + i * 3 + j] = B.element(i, 3 + j);       // DkMkt
        }
      SymmetricMatrix Bt(2); Bt = 0.0;
      ColumnVector At(6), X(6); At = 0.0;
      for (int k = 0; k < 6; k++) X.element(k) = X6[k];
      g->genBAtransForLinkedPair(1, 2, cm, cd, &Bt, &At, X);
      for (int k = 0; k < 6; k++) out[48 + k] = At.element(k);
      out[54] = Bt.element(0, 0); out[55] = Bt.element(0, 1); out[56] = Bt.element(1, 1);
      delete g;
    }
    return n;
  } catch (...) {
    return -1;
  }
}

void gb_rec_clear(void) { g_rec.clear(); }
int gb_rec_count(void) { return (int)g_rec.size(); }
int gb_rec_n(int i) { return g_rec[i].n; }
int gb_rec_get(int i, double* A, double* b, double* x)
{
  const Rec& r = g_rec[i];
  memcpy(A, r.A.data(), r.A.size() * sizeof(double)); memcpy(b, r.b.data(), r.n * sizeof(double));
  memcpy(x, r.x.data(), r.n * sizeof(double));
  return r.ok;
}

// doGraphSlam6D(gr, scans, nrIt) of back-end `backend`.  Returns 0, 1 on an exception.
int gb_run(int backend, int nscans, void** scans, int nlinks, const int* from, const int* to, double maxd, int nrIt, double* ret)
{
  omp_set_num_threads(1);
  Quiet q;
  try {
    std::vector<Scan*> all;
    for (int i = 0; i < nscans; i++) all.push_back((Scan*)scans[i]);
    Graph gr;
    for (int l = 0; l < nlinks; l++) gr.addLink(from[l], to[l]);
    gr.setNrScans(nscans);
    graphSlam6D* g = backend == 1 ? (graphSlam6D*)make<lum6DEuler>(maxd) : backend == 2 ? (graphSlam6D*)make<lum6DQuat>(maxd)
                     : backend == 3 ? (graphSlam6D*)make<ghelix6DQ2>(maxd) : (graphSlam6D*)make<gapx6D>(maxd);
    *ret = g->doGraphSlam6D(gr, all, nrIt);
    delete g;
    return 0;
  } catch (...) {
    return 1;
  }
}

}  // extern "C"
"""


def have_ref():
    return os.path.isfile(os.path.join(REF, "src", "slam6d", "lum6Dquat.cc"))


_lib = None
_tmp = None


def ref_lib():
    """the reference's sources + newmat + DRIVER, built into a temporary directory (removed at exit)"""
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="k16_ref_")
        d = _tmp.name
        for rel, text in (("slam6d/scan.h", SCAN_H), ("boost/graph/adjacency_list.hpp", BOOST_H), ("cs.h", CS_H)):
            p = os.path.join(d, "standin", rel)
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "w") as f:
                f.write(text)
        with open(os.path.join(d, "driver.cc"), "w") as f:
            f.write(DRIVER)
        # the stand-ins come first: "slam6d/scan.h" and <cs.h> resolve to them, everything else to the reference
        inc = ["-I" + os.path.join(d, "standin"), "-I" + os.path.join(REF, "include"),
               "-I" + os.path.join(REF, "3rdparty", "newmat", "newmat-10")]
        jobs, objs = [], []
        for s in SOURCES:
            objs.append(os.path.join(d, s + ".o"))
            jobs.append(["g++"] + FLAGS + inc + ["-c", os.path.join(REF, "src", "slam6d", s + ".cc"), "-o", objs[-1]])
        for s in NEWMAT:
            objs.append(os.path.join(d, "nm_" + s + ".o"))
            jobs.append(["g++", "-O2", "-fPIC", "-w", "-c",
                         os.path.join(REF, "3rdparty", "newmat", "newmat-10", "newmat", s + ".cpp"), "-o", objs[-1]])
        objs.append(os.path.join(d, "driver.o"))
        jobs.append(["g++"] + FLAGS + ["-fno-access-control"] + inc + ["-c", os.path.join(d, "driver.cc"), "-o", objs[-1]])
        width = max(1, min(16, os.cpu_count() or 1))
        for k in range(0, len(jobs), width):
            running = [subprocess.Popen(j) for j in jobs[k:k + width]]
            for r in running:
                if r.wait():
                    raise subprocess.CalledProcessError(r.returncode, r.args)
        so = os.path.join(d, "libgb.so")
        subprocess.check_call(["g++", "-shared", "-fopenmp", "-Wl,--no-undefined", "-o", so] + objs)
        L = C.CDLL(so)
        L.gb_scan_new.restype = C.c_void_p
        L.gb_scan_new.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint]
        L.gb_scan_free.argtypes = [C.c_void_p]
        L.gb_scan_pose.argtypes = [C.c_void_p, C.c_void_p]
        L.gb_pairs.restype = C.c_long
        L.gb_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_long, C.c_void_p, C.c_void_p]
        L.gb_link.restype = C.c_long
        L.gb_link.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        L.gb_rec_get.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gb_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p]
        _lib = L
    return _lib


class RefScan:
    def __init__(self, points, rPos=(0.0, 0.0, 0.0), rPosTheta=(0.0, 0.0, 0.0), nr=0):
        p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        rp, rt = np.array(rPos, np.float64), np.array(rPosTheta, np.float64)
        self.n = len(p)
        self.h = ref_lib().gb_scan_new(p.ctypes.data, len(p), rp.ctypes.data, rt.ctypes.data, nr)

    def pose(self):
        out = np.empty(POSE_WIDTH)
        ref_lib().gb_scan_pose(self.h, out.ctypes.data)
        return out

    def __del__(self):
        if self.h and _lib is not None:
            _lib.gb_scan_free(self.h)
            self.h = None


class Ref:
    """the reference's compiled back-ends"""

    @staticmethod
    def pairs(first, second, maxd):
        p1 = np.empty((second.n, 3)); p2 = np.empty((second.n, 3))
        n = ref_lib().gb_pairs(first.h, second.h, float(maxd) * float(maxd), second.n, p1.ctypes.data, p2.ctypes.data)
        return p1[:n].copy(), p2[:n].copy()

    @staticmethod
    def link(backend, first, second, maxd, X6=None):
        """-> (number of pairs, LINK_WIDTH[backend] doubles)"""
        out = np.zeros(LINK_WIDTH[backend])
        x6 = np.zeros(6) if X6 is None else np.ascontiguousarray(X6, np.float64)
        n = ref_lib().gb_link(backend, first.h, second.h, float(maxd), x6.ctypes.data, out.ctypes.data)
        if n < 0:
            raise RuntimeError("the reference threw")
        return int(n), out

    @staticmethod
    def run(backend, scans, links, maxd, nrIt):
        """doGraphSlam6D -> (ret, [(A, rhs, X, ok) per cs_cholsol call])"""
        L = ref_lib()
        L.gb_rec_clear()
        hs = (C.c_void_p * len(scans))(*[s.h for s in scans])
        frm = np.array([a for a, _ in links], np.int32); to = np.array([b for _, b in links], np.int32)
        ret = C.c_double(0.0)
        rc = L.gb_run(backend, len(scans), hs, len(links), frm.ctypes.data, to.ctypes.data, float(maxd), int(nrIt), C.byref(ret))
        if rc:
            raise RuntimeError("the reference threw")
        recs = []
        for i in range(L.gb_rec_count()):
            n = L.gb_rec_n(i)
            A = np.empty((n, n)); b = np.empty(n); x = np.empty(n)
            ok = L.gb_rec_get(i, A.ctypes.data, b.ctypes.data, x.ctypes.data)
            recs.append((A, b, x, int(ok)))
        return float(ret.value), recs


def pair_sha(p1, p2):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(p1, np.float64).tobytes()); h.update(np.ascontiguousarray(p2, np.float64).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def runs_in_reference(g, backend, npairs):
    """lum6DQuat on a link of fewer than 3 pairs ends the process (see the docstring)"""
    return not (backend == 2 and min(npairs) < gc.MIN_PAIRS[2])


def compute_link(name):
    model, data, maxd = gc.link_case(name)
    a, b = RefScan(model), RefScan(data, nr=1)
    p1, p2 = Ref.pairs(a, b, maxd)
    z = {"link_%s_n" % name: np.array(len(p1), np.int64), "link_%s_sha" % name: pair_sha(p1, p2)}
    want = gc.link_pairs_expected(name)
    assert want is None or want == len(p1), (name, len(p1))
    assert want is not None or len(p1) > 0.9 * gc.N_LINK, (name, len(p1))
    for k in gc.BACKENDS:
        n, out = Ref.link(k, a, b, maxd, TRANS_X)
        assert n == len(p1)
        z["link_%s_b%d" % (name, k)] = out
    return z


def ref_scans(g):
    return [RefScan(g.points[i], g.rPos[i], g.rPosTheta[i], nr=i) for i in range(g.nscans)]


def _blocks(backend, scans, links, maxd):
    out = np.zeros((len(links), LINK_WIDTH[backend])); npairs = np.zeros(len(links), np.int64)
    for l, (f, t) in enumerate(links):
        npairs[l], out[l] = Ref.link(backend, scans[f], scans[t], maxd)
    return out, npairs


def scatter(k, links, blocks, npairs, n, state=None, assign=True, first_scan=True, thresholds=True):
    """the four scatter rules restated (lum6Deuler.cc:265-303, lum6Dquat.cc:246-276, ghelix6DQ2.cc:158-284,
    gapx6D.cc:281-307) over the reference's per-link quantities (LINK_LAYOUT) -> (A, rhs); the switches turn single rules
    off.  state: ghelix6DQ2's (B, bd) / gapx6D's (B, what the translation step left in A) of the previous iteration, or None."""
    w = {1: 6, 2: 7, 3: 6, 4: 3}[k]
    N = w * n
    A = np.zeros((N, N)) if state is None else state[0].copy()
    rhs = np.zeros(N) if state is None else state[1].copy()
    lay = LINK_LAYOUT[k]
    for l, (f, t) in enumerate(links):
        if thresholds and npairs[l] < gc.MIN_PAIRS[k]:
            continue
        b = blocks[l]
        a, c = (f - 1) * w, (t - 1) * w
        if not first_scan and f == 0 and l != 0:
            continue                            # (rule off: the links out of the fixed scan, but for the first, are dropped)
        if k <= 2:
            Cab, CD = b[lay["C"]].reshape(w, w), b[lay["CD"]]
            if f != 0:
                rhs[a:a + w] += CD; A[a:a + w, a:a + w] += Cab
            if t != 0:
                rhs[c:c + w] -= CD; A[c:c + w, c:c + w] += Cab
            if f != 0 and t != 0:
                if k == 2 and assign:
                    A[a:a + w, c:c + w] = -Cab; A[c:c + w, a:a + w] = -Cab
                else:
                    A[a:a + w, c:c + w] -= Cab; A[c:c + w, a:a + w] -= Cab
        elif k == 3:
            Blk, bd1, bd2 = b[lay["Blk"]].reshape(6, 6), b[lay["bd1"]], b[lay["bd2"]]
            if f != 0:
                A[a:a + 6, a:a + 6] += Blk; rhs[a:a + 6] += bd1
            A[c:c + 6, c:c + 6] += Blk; rhs[c:c + 6] += bd2
            if f != 0:
                A[a:a + 6, c:c + 6] -= Blk; A[c:c + 6, a:a + 6] -= Blk
        else:
            if f != 0:
                rhs[a:a + 3] += b[lay["Ak1"]]
                A[a:a + 3, a:a + 3] += b[lay["MkMkt"]].reshape(3, 3)
                A[a:a + 3, c:c + 3] += b[lay["DkMkt"]].reshape(3, 3)
                A[c:c + 3, a:a + 3] += b[lay["MkDkt"]].reshape(3, 3)
            rhs[c:c + 3] += b[lay["Ak2"]]
            A[c:c + 3, c:c + 3] += b[lay["DkDkt"]].reshape(3, 3)
    return A, rhs


def dropped(A, drop=True):
    return np.where(np.abs(A) > 0.00001, A, 0.0) if drop else A.copy()


def compute_graph(name, backend):
    g = gc.graph(name)
    links = g.links(backend)
    key = "graph_%s_b%d_" % (name, backend)
    z = {}
    s1 = ref_scans(g)
    z[key + "blocks_it1"], z[key + "npairs_it1"] = _blocks(backend, s1, links, g.maxd)
    if not runs_in_reference(g, backend, z[key + "npairs_it1"]):
        z[key + "status"] = np.array(-1, np.int64)
        return z
    z[key + "status"] = np.array(0, np.int64)
    ret1, rec1 = Ref.run(backend, s1, links, g.maxd, 1)
    z[key + "ret1"] = np.array(ret1)
    z[key + "poses1"] = np.array([s.pose() for s in s1])
    z[key + "blocks_it2"], z[key + "npairs_it2"] = _blocks(backend, s1, links, g.maxd)
    s2 = ref_scans(g)
    ret2, rec2 = Ref.run(backend, s2, links, g.maxd, 2)
    z[key + "ret2"] = np.array(ret2)
    z[key + "poses2"] = np.array([s.pose() for s in s2])
    assert len(rec1) == 1 and len(rec2) == 2
    for a, b in zip(rec1[0][:3], rec2[0][:3]):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    if backend in gc.DROP_GRAPHS.get(name, ()):
        # the graph is there for the drop rule: its assembled matrix has nonzero entries with |v| <= 1e-5.  The reference
        # drops them before cs_entry sees them, so the matrix is assembled here, from the reference's own blocks, and shown
        # to be, after the drop, the one cs_cholsol was handed, bit for bit
        A0 = scatter(backend, links, z[key + "blocks_it1"], z[key + "npairs_it1"], g.nscans - 1)[0]
        assert ((A0 != 0) & (np.abs(A0) <= 0.00001)).any(), (name, backend)
        assert np.array_equal(dropped(A0).view(np.uint64), rec2[0][0].view(np.uint64)), (name, backend)
    for j, (A, b, x, ok) in enumerate(rec2):
        assert ok == 1, (name, backend, j, "the stand-in Cholesky found the matrix not positive definite")
        z[key + "it%d_A" % (j + 1)] = A; z[key + "it%d_rhs" % (j + 1)] = b; z[key + "it%d_X" % (j + 1)] = x
    return z


def compute():
    z = {}
    for name in gc.LINK_CASES:
        z.update(compute_link(name))
    for name in gc.GRAPHS:
        for k in gc.BACKENDS:
            z.update(compute_graph(name, k))
    return z


def load(path=OUT):
    return dict(np.load(path))


def save(z, path=OUT):
    """np.savez_compressed with nothing in the file that depends on when it was written"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for k in sorted(z):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(z[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue(), compresslevel=9)


if __name__ == "__main__":
    if not have_ref():
        raise SystemExit("needs the reference checkout at %s (src/slam6d/lum6Dquat.cc)" % REF)
    z = compute()
    save(z)
    size = os.path.getsize(OUT)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(z), size))
    assert size <= MAX_BYTES, size
