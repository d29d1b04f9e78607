// LAB ONLY (lib3dtk_hip_lab.so; a measured negative, NEGATIVES.md): the records of the two-levels-per-trip walks (KdFat: a node and
// both its children in one record; lab_fat_walk.inc and lab_fat_small.inc read them), made from the finished tree.
__global__ void __launch_bounds__(256) k_make_fat(const KdNode* __restrict__ nodes, size_t n, KdFat* __restrict__ fat)
{
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const KdNode nd = nodes[i];
  KdFat f;
  memset(&f, 0, sizeof f);
  f.cx = (float)nd.cx; f.cy = (float)nd.cy; f.cz = (float)nd.cz; f.hx = (float)nd.hx; f.hy = (float)nd.hy; f.hz = (float)nd.hz;
  f.c1 = nd.c1; f.c2 = nd.c2; f.splitval = nd.splitval;
  if (!(nd.c1 & REF_LEAF)) {
    const KdNode a = nodes[nd.c1 & REF_VAL];
    f.a_cx = (float)a.cx; f.a_cy = (float)a.cy; f.a_cz = (float)a.cz; f.a_hx = (float)a.hx; f.a_hy = (float)a.hy; f.a_hz = (float)a.hz;
    f.a_split = a.splitval; f.a_c1 = a.c1; f.a_c2 = a.c2;
  }
  if (!(nd.c2 & REF_LEAF)) {
    const KdNode b = nodes[nd.c2 & REF_VAL];
    f.b_cx = (float)b.cx; f.b_cy = (float)b.cy; f.b_cz = (float)b.cz; f.b_hx = (float)b.hx; f.b_hy = (float)b.hy; f.b_hz = (float)b.hz;
    f.b_split = b.splitval; f.b_c1 = b.c1; f.b_c2 = b.c2;
  }
  fat[i] = f;
}
hipError_t launch_make_fat(const KdNode* nodes, size_t n, KdFat* fat, hipStream_t s)
{
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_make_fat, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, nodes, n, fat);
  return hipGetLastError();
}
