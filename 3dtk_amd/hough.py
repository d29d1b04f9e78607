"""The standard 3D Hough transform for plane detection (src/shapes: Hough::SHT, the four accumulators) on the device, up to
plane candidates.  A thin mirror over tdtk_hough_*: the vote for every cell of the accumulator, the sorted peak list, the
plane a cell stands for, the points within MaxPointPlaneDist of a plane and the least-squares plane through them.  Not
covered: the randomized variants (RHT, PHT, PPHT, APHT), peakWindow, and the second half of deletePoints (projection,
clustering, convex hull and the deletion of points between peaks)."""
import ctypes as C
import re

import numpy as np

from ._capi import lib, check, dptr, iptr, f64

SIMPLE, BALL, CUBE, BALLI = 0, 1, 2, 3


class ConfigFileHough:
    """ConfigFileHough (include/shapes/ConfigFileHough.h:4-24): the reference's field names and defaults"""
    _FIELDS = (("MaxDist", float, 500.0), ("MinDist", float, 50.0), ("AccumulatorMax", int, 100), ("MinSizeAllPoints", int, 20),
               ("RhoNum", int, 500), ("ThetaNum", int, 360), ("PhiNum", int, 176), ("RhoMax", int, 1500),
               ("MaxPointPlaneDist", float, 1.5), ("MaxPlanes", int, 20), ("MinPlaneSize", int, 100), ("MinPlanarity", float, 0.3),
               ("PlaneRatio", float, 0.5), ("PointDist", float, 5.0), ("PeakWindow", int, 0), ("WindowSize", int, 8),
               ("TrashMax", int, 20), ("AccumulatorType", int, 3))

    def __init__(self, **kw):
        self.CfgFileName = "bin/hough.cfg"
        self.PlaneDir = "dat/planes/"
        for name, kind, default in self._FIELDS:
            setattr(self, name, kind(default))
        self.PeakWindow = False
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError("ConfigFileHough has no field %r" % k)
            setattr(self, k, v)

    def LoadCfg(self, path):
        """ConfigFileHough::LoadCfg over parascan.cc's `Name value` files: a field's value is the token behind the first
        occurrence of its name outside a comment (# to the end of the line); a name that does not occur keeps the default.
        Returns 0, or -1 when the file cannot be opened (the reference prints and returns)."""
        try:
            with open(path) as f:
                text = re.sub(r"#[^\n]*\n", "", f.read())
        except OSError:
            return -1

        def token(name):
            at = text.find(name)
            if at < 0:
                return None
            rest = text[at + len(name) + 1:].split()
            return rest[0] if rest else None

        def number(tok, kind):                     # atoi / atof: the longest numeric prefix, 0 without one
            pat = r"\s*[+-]?\d+" if kind is int else r"\s*[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?)"
            m = re.match(pat, tok)
            return kind(m.group(0)) if m else kind(0)
        for name, kind, _ in self._FIELDS:
            tok = token(name)
            if tok is not None:
                setattr(self, name, number(tok, kind))
        self.PeakWindow = bool(self.PeakWindow)
        tok = token("PlaneDir")
        if tok is not None:
            self.PlaneDir = tok
        self.CfgFileName = str(path)
        return 0

    def dims(self):
        return np.array([self.RhoNum, self.PhiNum, self.ThetaNum, self.RhoMax], np.uint32)


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def hough_normals(cfg):
    """(normals [C][3], slice_sizes): the normal every cell of cfg's accumulator votes with (tdtk_hough_normals), in the order
    of that accumulator's getMax() loops without the rho loop, and the cells per phi slice (AccumulatorCube: per face)"""
    dims = cfg.dims()
    n = C.c_size_t(0)
    sizes = np.zeros(6 if cfg.AccumulatorType == CUBE else max(int(cfg.PhiNum), 1), np.int32)
    check(lib().tdtk_hough_normals(int(cfg.AccumulatorType), _u32p(dims), None, 0, C.byref(n), iptr(sizes)))
    normals = np.empty((n.value, 3), np.float64)
    check(lib().tdtk_hough_normals(int(cfg.AccumulatorType), _u32p(dims), dptr(normals), n.value, C.byref(n), iptr(sizes)))
    return normals, sizes


class Hough:
    """Hough(points, cfg): the reference's Hough object as far as the standard transform goes.  Every method hands the cloud
    to the library again, except inside SHT(), whose steps follow each other on one thread: there the cloud is uploaded once
    and the peaks are read from the vote's counts where they lie on the device."""

    def __init__(self, points, cfg=None, device=0):
        self.cfg = cfg if cfg is not None else ConfigFileHough()
        self.points = f64(points).reshape(-1, 3)
        self.device = device
        self.normals, self.slice_sizes = hough_normals(self.cfg)
        self._counts = None
        self._resident = False       # inside SHT(), behind its vote: the thread's device context holds this cloud and its counts

    def _xyz(self):
        """the argument for `xyz`: the host array, or NULL (the cloud the thread uploaded last) inside SHT()"""
        return None if self._resident else dptr(self.points)

    def votes(self):
        """counts [C][RhoNum] int32: accumulate(Point) of every point (Hough::SHT, hough.cc:236-244), the reference's counts
        cell for cell; counts[c][k] is cell c of the normals table, rho bin k"""
        cfg = self.cfg
        counts = np.empty((len(self.normals), int(cfg.RhoNum)), np.int32)
        check(lib().tdtk_hough_vote(self.device, self._xyz(), len(self.points), dptr(self.normals), len(self.normals),
                                    int(cfg.RhoNum), int(cfg.RhoMax), float(cfg.MaxPointPlaneDist), iptr(counts)))
        self._counts = counts
        return counts

    def peaks(self, max_planes=None):
        """the head of getMax()'s sorted list that Hough::SHT walks (hough.cc:246-263): the cells with count > (int)(max *
        PlaneRatio), at most max_planes (default cfg.MaxPlanes) of them: [n][4] (count, rho, theta, phi), AccumulatorCube
        [n][5] (count, rho, face, i, j)"""
        if self._counts is None:
            self.votes()
        cfg = self.cfg
        width = 5 if cfg.AccumulatorType == CUBE else 4
        n, mx = C.c_uint64(0), C.c_int32(0)
        dims = cfg.dims()
        src = None if self._resident else iptr(self._counts)      # NULL: the counts of the thread's last vote, in place
        L = lib()
        rc = L.tdtk_hough_peaks(self.device, src, int(cfg.AccumulatorType), _u32p(dims), float(cfg.PlaneRatio), None, 0,
                                C.byref(n), C.byref(mx))
        if n.value == 0:
            check(rc)
            return np.zeros((0, width), np.int32)
        cells = np.empty((n.value, width), np.int32)
        check(L.tdtk_hough_peaks(self.device, None, int(cfg.AccumulatorType), _u32p(dims), float(cfg.PlaneRatio),
                                 iptr(cells), n.value, C.byref(n), C.byref(mx)))
        k = int(cfg.MaxPlanes) if max_planes is None else int(max_planes)
        return cells[:k] if k >= 0 else cells

    def cell_plane(self, cell):
        """getMax(int* cell): (nx, ny, nz, rho) of the plane at the centre of a cell.  For AccumulatorCube the reference reads
        the entry as (rho, face - 1, i, j), not as peaks() lists it; cube_cell() converts."""
        cell = np.ascontiguousarray(cell, np.int32)
        plane = np.zeros(4)
        dims = self.cfg.dims()
        check(lib().tdtk_hough_cell_plane(int(self.cfg.AccumulatorType), _u32p(dims), iptr(cell), dptr(plane)))
        return plane

    @staticmethod
    def cube_cell(entry):
        """an AccumulatorCube entry of peaks() (count, rho, face, i, j) as the array its getMax(int*) reads so that it lands
        on that cell's centre: (rho, face, i + 1, j + 1, 0)"""
        e = np.asarray(entry, np.int32)
        return np.array([e[1], e[2], e[3] + 1, e[4] + 1, 0], np.int32)

    def plane_points(self, n, rho):
        """deletePoints' first loop (hough.cc:759-779): (mask [N] bool, indices in input order) of the points with
        |p . n/|n| - rho| < MaxPointPlaneDist"""
        nn = f64(n).reshape(3)
        N = len(self.points)
        mask = np.zeros(N, np.uint8)
        cnt = C.c_uint64(0)
        L = lib()
        D = float(self.cfg.MaxPointPlaneDist)
        mp = mask.ctypes.data_as(C.POINTER(C.c_uint8))
        check(L.tdtk_hough_plane_points(self.device, self._xyz(), N, dptr(nn), float(rho), D, mp, None, 0, C.byref(cnt)))
        idx = np.empty(cnt.value, np.int32)
        if cnt.value:
            check(L.tdtk_hough_plane_points(self.device, self._xyz(), N, dptr(nn), float(rho), D, mp, iptr(idx), cnt.value,
                                            C.byref(cnt)))
        return mask.astype(bool), idx

    def fit_plane(self, indices):
        """calcPlane (hough.cc:1252-1310) over points[indices]: (plane [4] = unit normal and n . centroid, planarity); fewer
        than three points: (None, 0.0)"""
        idx = np.ascontiguousarray(indices, np.int32).reshape(-1)
        plane = np.zeros(4)
        pl = C.c_double(0.0)
        check(lib().tdtk_hough_fit_plane(self.device, self._xyz(), len(self.points), iptr(idx), len(idx), dptr(plane), C.byref(pl)))
        if len(idx) < 3:
            return None, 0.0
        return plane, pl.value

    def SHT(self):
        """Plane CANDIDATES of the standard Hough transform: for every peak, over the undiminished cloud, a dict with the
        cell, its plane (cell_plane), the inlier count and indices (plane_points), the refitted plane and its planarity
        (fit_plane).  These are not the reference's final ConvexPlanes: Hough::SHT deletes each plane's clustered points
        before it looks at the next peak (the second half of deletePoints: projection, clustering, Jarvis march), so its
        later planes are found in a smaller cloud; here nothing is deleted between peaks."""
        self.votes()
        self._resident = True
        try:
            return self._candidates()
        finally:
            self._resident = False

    def _candidates(self):
        out = []
        for entry in self.peaks():
            cell = self.cube_cell(entry) if self.cfg.AccumulatorType == CUBE else entry
            plane = self.cell_plane(cell)
            _, idx = self.plane_points(plane[:3], plane[3])
            fit, planarity = self.fit_plane(idx)
            out.append(dict(cell=entry.copy(), plane=plane, inliers=len(idx), indices=idx, fit=fit, planarity=planarity))
        return out


def last_timings():
    """HIP-event times of this thread's last vote, peaks, plane_points and fit_plane, ms, and how often the Hough device
    buffers were (re)allocated"""
    ms = np.zeros(5)
    check(lib().tdtk_hough_timings(dptr(ms)))
    return dict(vote_ms=ms[0], peaks_ms=ms[1], plane_points_ms=ms[2], fit_ms=ms[3], allocations=int(ms[4]))
