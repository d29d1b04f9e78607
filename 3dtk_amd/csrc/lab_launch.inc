// LAB ONLY (lib3dtk_hip_lab.so): the launch policy of the measured negatives (NEGATIVES.md) -- the configurations of the persistent-lane
// kernels that only the lab builds, the grids of the experiments, and one hook per product launch function (kernels.hip), which either
// makes the lab's launch and says so or declines.  Every experiment is selected by its environment switch; with none set every hook declines.
// ---- configurations: each experiment overrides the members that make it that experiment ----
// the experiments that change the workgroup or the hand-out were built on the plain kernel: four LDS levels, four waves per SIMD
template <bool COUNT_, int FUSE_> struct LabPlain : RefillCfg { static constexpr bool COUNT = COUNT_; static constexpr int FUSE = FUSE_; };
// TDTK_TOP_BLOCK: the first TOP_ hot records in LDS, one copy per workgroup of BLOCK_ threads (TOP_ 0: the workgroup size alone)
template <bool COUNT_, int FUSE_, int BLOCK_, int TOP_> struct LabTop : LabPlain<COUNT_, FUSE_> { static constexpr int BLOCK = BLOCK_, TOP = TOP_; };
// TDTK_SHARE_BLOCK: the waves of a workgroup of BLOCK_ threads hand out one slab together
template <bool COUNT_, int FUSE_, int BLOCK_> struct LabShare : LabPlain<COUNT_, FUSE_> { static constexpr int BLOCK = BLOCK_; static constexpr bool SHARE = true; };
template <bool COUNT_, int FUSE_> struct LabWave : LabPlain<COUNT_, FUSE_> { static constexpr int BLOCK = 64; };      // TDTK_SINGLE_BLOCK=64: workgroups of one wave
// TDTK_PIPE=1: the hand-out that does not wait (SD_: the LDS levels of the launch it replaces)
template <bool COUNT_, int FUSE_, int SD_> struct LabPipe : LabPlain<COUNT_, FUSE_> { static constexpr int SD = SD_; static constexpr bool PIPE = true; };
// the experiments inside the walk and the bucket scan: the timed FUSE 0 kernel with the compiler's own register count
// (SD_: the LDS levels of the launch they stand in for)
template <int SD_> struct LabOwnRegs : RefillCfg { static constexpr int SD = SD_, WPS = 1; };
template <int SD_> struct LabPts8 : LabOwnRegs<SD_> { static constexpr int PTS = 8; };                      // TDTK_BUCKET_PTS=8
template <int SD_, int PROBE_> struct LabProbe : LabOwnRegs<SD_> { static constexpr int PROBE = PROBE_; };   // TDTK_BUCKET_PTS=41|42|43
template <int SD_> struct LabFat : LabOwnRegs<SD_> { static constexpr bool FAT = true; };                   // TDTK_FAT_NODES=1
template <bool COUNT_, int FUSE_> struct LabThresh8 : LabOwnRegs<REFILL_SD<FUSE_>> { static constexpr int THRESH = 8, FUSE = FUSE_; static constexpr bool COUNT = COUNT_; };   // TDTK_REFILL_THRESH=8
// FUSE 1 / 2 (TDTK_FUSE_SUMS): the sums at every retire / the graph-SLAM link's sums, in the product's launch otherwise
template <int THRESH_, bool COUNT_, int FUSE_> struct LabFuse : RefillCfg {
  static_assert(FUSE_ == 1 || FUSE_ == 2, "0 and 3 are the product's: SinglePass");
  static constexpr int THRESH = THRESH_, WPS = REFILL_WPS<COUNT_, FUSE_>, FUSE = FUSE_; static constexpr bool COUNT = COUNT_;
};
// TDTK_SEARCH_VARIANT=30: slabs drawn from a work queue (nothing to order then)
template <int THRESH_, bool COUNT_> struct LabQueue : RefillCfg { static constexpr int THRESH = THRESH_, WPS = 1; static constexpr bool COUNT = COUNT_, DYN = true, ORDER = false; };
struct LabBlock256 : RefillCfg { static constexpr int BLOCK = SEARCH_BLOCK, WPS = 1; };      // TDTK_SEARCH_VARIANT=8: 256-thread workgroups
// the several-links launch: TDTK_REFILL_THRESH=8, TDTK_MULTI_BLOCK=64 (workgroups of one wave), TDTK_PIPE=1
template <bool COUNT_, bool ORDER_> struct LabLinkThresh8 : LinkPass<16, COUNT_, 0, ORDER_, 4> { static constexpr int THRESH = 8; };
template <int THRESH_> struct LabLinkWave : LinkPass<THRESH_, false, 5, true, 4> { static constexpr int BLOCK = 64, SD = 4; };
template <int THRESH_> struct LabLinkPipe : LinkPass<THRESH_, false, 5, true, 4> { static constexpr bool PIPE = true; };
// ---- switches and grids ----
static uint32_t refill_grid_b_fwd(size_t n, int* qpw_out) { return refill_grid_b(n, 128, qpw_out); }      // (for lab_slab_bounds.inc)
// what the big-workgroup and single-wave experiments share: only while the launch is ONE generation of resident waves with the
// chip to itself, and with none of the switches in `others` set
static bool lab_one_generation_alone(size_t n, int side_by_side, std::initializer_list<const char*> others)
{
  if (side_by_side > 1 || (n + 255) / 256 >= (size_t)num_cu() * 4 * 7) return false;
  for (const char* name : {"TDTK_REFILL_POOL", "TDTK_BUCKET_PTS", "TDTK_FAT_NODES", "TDTK_WAVE_TRACE", "TDTK_REFILL_THRESH", "TDTK_TWO_PER_LANE",
                           "TDTK_FUSE_SUMS", "TDTK_SEARCH_VARIANT", "TDTK_REFILL_QPW"})
    if (lab_env(name)) return false;
  for (const char* name : others)
    if (lab_env(name)) return false;
  return true;
}
// Upper tree levels in LDS (LabTop): the workgroup size of the single-pass launch that stages them, 0 = the plain 128-thread
// kernel.  A big workgroup leaves its CU when its slowest wave does, which costs nothing when nobody is waiting for the CU.
// MEASURED NEGATIVE (TDTK_TOP_BLOCK=512|1024): 1M-vs-1M k_search 0.2041-0.2047 ms (1024) / 0.2071-0.2080 (512)
// against 0.1933-0.1945; the upper levels' visits coalesce in the vector L1 anyway -- a wave's sorted queries share their
// first ten nodes -- so LDS takes little off the tag pipeline and the mixed trips pay for two paths.
static int refill_top_block(size_t n, int side_by_side)
{
  const char* e = lab_env("TDTK_TOP_BLOCK");
  const int blk = e ? atoi(e) : 0;
  if (blk != 128 && blk != 512 && blk != 1024) return 0;      // (128: seven levels per 128-thread workgroup; TDTK_TOP_LEVELS=0 with 1024: no staging, the workgroup size alone)
  return lab_one_generation_alone(n, side_by_side, {}) ? blk : 0;
}
// Slabs handed out by the workgroup's waves together (LabShare): the workgroup size of the single-pass launch, 0 = every wave
// for itself (128-thread workgroups).
// MEASURED NEGATIVE (TDTK_SHARE_BLOCK=256|512|1024): 1M-vs-1M k_search 0.2075-0.2085 / 0.2171-0.2179 / 0.2121-0.2131 ms
// against 0.1945-0.1956: the waves of a big workgroup sit on ONE CU and share its vector L1, which is what the kernel is
// bound by (TCP busy 80-91 % of the launch, profiles/r04_tcp_diag.txt); 128-thread workgroups spread a CU's sixteen waves
// over eight distant stretches of the scan, and that averaging is worth more than what the shared cursor evens out.
static int refill_share_block(size_t n, int side_by_side)
{
  int blk = 0;
  if (const char* e = lab_env("TDTK_SHARE_BLOCK")) blk = atoi(e);
  if (blk != 256 && blk != 512 && blk != 1024) return 0;
  return lab_one_generation_alone(n, side_by_side, {"TDTK_TOP_BLOCK", "TDTK_REFILL_PHASES", "TDTK_BALANCE"}) ? blk : 0;
}
// TDTK_SINGLE_BLOCK=64: the single-pass launch in workgroups of ONE wave (a CU's sixteen waves then come from sixteen
// distant stretches of the scan instead of eight)
static bool refill_single64(size_t n, int side_by_side)
{
  const char* e = lab_env("TDTK_SINGLE_BLOCK");
  if (!(e && atoi(e) == 64)) return false;
  return lab_one_generation_alone(n, side_by_side, {"TDTK_TOP_BLOCK", "TDTK_REFILL_PHASES", "TDTK_BALANCE", "TDTK_SHARE_BLOCK", "TDTK_PIPE"});
}
// the workgroup size of the single-pass launch where it is a big one (0: it is not)
static int refill_big_block(size_t n, int side_by_side)
{
  if (const int tb = refill_top_block(n, side_by_side)) return tb;
  return refill_share_block(n, side_by_side);
}
// two queries per lane (k_search_refill2, TDTK_TWO_PER_LANE=<waves per SIMD: 2 or 3>): one generation of that many waves
static int two_per_lane()
{
  const char* e = lab_env("TDTK_TWO_PER_LANE");
  const int v = e ? atoi(e) : 0;
  return (v == 2 || v == 3) ? v : 0;
}
static uint32_t refill2_grid(size_t n, int* qpw_out)
{
  const size_t slots = (size_t)num_cu() * 4 * (size_t)two_per_lane();
  size_t qpw = (n + slots - 1) / slots;
  qpw = (qpw + 31) & ~(size_t)31;
  if (qpw < 128) qpw = 128;
  if (qpw > 512) qpw = 512;
  const size_t waves = (n + qpw - 1) / qpw;
  size_t nb = (waves + 1) / 2;
  nb = (nb + 7) & ~(size_t)7;
  *qpw_out = (int)qpw;
  return (uint32_t)(nb < 8 ? 8 : nb);
}
static bool two_per_lane_for(size_t n, int side_by_side)
{
  return two_per_lane() && side_by_side <= 1 && pick_variant(n) == 20 && (n + 511) / 512 <= (size_t)num_cu() * 4 * (size_t)two_per_lane();
}
// pipelined hand-out (LabPipe, LabLinkPipe; TDTK_PIPE=1).  MEASURED NEGATIVE: parity-green, and the bucket scan -- where the
// register demand peaks -- finds 8-9 more registers live with it (phi copies of the query registers the staged loads land in):
// 134 VGPRs = three waves per SIMD, or at 128 nine spilled registers in hot code: 1M-vs-1M k_search 0.2348 ms against
// 0.1954-0.1959, one lum6DEuler round of 84 links 13.9 ms against 10.5.
static bool pipe_on()
{
  if (const char* e = lab_env("TDTK_PIPE")) return e[0] == '1';
  return false;
}
// TDTK_MULTI_BLOCK=64: the several-links launch in workgroups of ONE wave -- a wave slot is free again when its wave is done, not
// when its workgroup's slower wave is (the rows of partial sums are then one per wave)
static bool multi_block64()
{
  const char* e = lab_env("TDTK_MULTI_BLOCK");
  return e && atoi(e) == 64;
}
// work-queue kernel: as many waves as stay resident (TDTK_STREAM_WPS per SIMD, default 7 = what the registers allow),
// never more waves than there are slabs to draw
static int stream_slab_env()
{
  const char* e = lab_env("TDTK_STREAM_SLAB");
  return std::max(16, e ? atoi(e) : 256);
}
static uint32_t stream_grid(size_t n)
{
  const char* e = lab_env("TDTK_STREAM_WPS");
  const int wps = std::min(8, std::max(1, e ? atoi(e) : 4));
  size_t waves = (size_t)num_cu() * 4 * (size_t)wps;
  const size_t slabs = (n + (size_t)stream_slab_env() - 1) / (size_t)stream_slab_env();
  if (waves > slabs) waves = slabs;
  size_t nb = (waves + 1) / 2;          // 128-thread workgroups
  return (uint32_t)(nb ? nb : 1);
}
// ---- the grid queries' hooks (0: the product's answer holds) ----
static size_t lab_max_lanes(size_t n)
{
  const int tb = refill_big_block(n, 1);
  if (!tb) return 0;
  int q;
  const size_t t = (size_t)refill_grid_b(n, tb, &q) * (size_t)tb;
  const size_t a0 = (size_t)search_grid(n) * SEARCH_BLOCK, b0 = (size_t)refill_grid_b(n, 128, &q) * 128;
  return std::max(t, std::max(a0, b0));
}
static uint32_t lab_fused_rows(size_t n, int side_by_side)
{
  int q;
  if (two_per_lane_for(n, side_by_side)) return refill2_grid(n, &q);
  if (const int tb = refill_big_block(n, side_by_side)) return refill_grid_b(n, tb, &q, side_by_side) * (uint32_t)(tb / 128);
  if (refill_single64(n, side_by_side)) return refill_grid_b(n, 64, &q, side_by_side);
  return 0;
}
// ---- launch_refill128's hooks ----
// before the product's grid: the experiments that bring a grid of their own (upper levels in LDS, single-wave workgroups,
// shared slabs, two queries per lane)
template <bool COUNT, int FUSE>
static bool lab_refill_own_grid(SearchArgs& a, hipStream_t s)
{
  if constexpr (FUSE == 0 || FUSE == 3) {
    int qpw;
    const auto one_piece = [&] { a.qpw = qpw; a.phases = 1; a.pool_slab = 0; a.region = 0; a.trace = 0; };
    const int tb = a.bounds ? 0 : refill_top_block(a.n, a.side_by_side);
    const bool wave = !tb && !a.bounds && refill_single64(a.n, a.side_by_side);
    const int sb = (tb || wave || a.bounds) ? 0 : refill_share_block(a.n, a.side_by_side);
    if (const int blk = tb ? tb : (wave ? 64 : sb)) {
      const uint32_t nb = refill_grid_b(a.n, blk, &qpw, a.side_by_side);
      one_piece();
      const char* lv = lab_env("TDTK_TOP_LEVELS");
      if (tb == 1024 && lv && lv[0] == '0') launch_refill<LabTop<COUNT, FUSE, 1024, 0>>(nb, 0, s, a);
      else if (tb == 128) launch_refill<LabTop<COUNT, FUSE, 128, 127>>(nb, 0, s, a);
      else if (tb == 1024) launch_refill<LabTop<COUNT, FUSE, 1024, 1023>>(nb, 0, s, a);
      else if (tb) launch_refill<LabTop<COUNT, FUSE, 512, 511>>(nb, 0, s, a);
      else if (wave) launch_refill<LabWave<COUNT, FUSE>>(nb, 0, s, a);
      else if (sb == 1024) launch_refill<LabShare<COUNT, FUSE, 1024>>(nb, 0, s, a);
      else if (sb == 512) launch_refill<LabShare<COUNT, FUSE, 512>>(nb, 0, s, a);
      else launch_refill<LabShare<COUNT, FUSE, 256>>(nb, 0, s, a);
      return true;
    }
    if (two_per_lane_for(a.n, a.side_by_side) && !a.bounds && !a.skip) {
      const uint32_t nb2 = refill2_grid(a.n, &qpw);
      one_piece();
      const char* e1 = lab_env("TDTK_TWO_ONE");
      if (e1 && e1[0] == '1') {
        if (two_per_lane() == 3) hipLaunchKernelGGL((k_search_refill2<128, 4, 16, COUNT, FUSE, 3, true>), dim3(nb2), dim3(128), 0, s, a);
        else hipLaunchKernelGGL((k_search_refill2<128, 4, 16, COUNT, FUSE, 2, true>), dim3(nb2), dim3(128), 0, s, a);
      } else if (two_per_lane() == 3) hipLaunchKernelGGL((k_search_refill2<128, 4, 16, COUNT, FUSE, 3>), dim3(nb2), dim3(128), 0, s, a);
      else hipLaunchKernelGGL((k_search_refill2<128, 4, 16, COUNT, FUSE, 2>), dim3(nb2), dim3(128), 0, s, a);
      return true;
    }
  }
  return false;
}
// on the product's grid (nb workgroups of 128 threads, lds bytes of unused dynamic LDS): the experiments inside the walk and
// the bucket scan, the hand-out threshold of 8, the pipelined hand-out, the FUSE values the product does not launch
template <bool COUNT, int FUSE>
static bool lab_refill_on_grid(const SearchArgs& a, uint32_t nb, unsigned lds, hipStream_t s)
{
  const char* pe = lab_env("TDTK_BUCKET_PTS");      // 8 scans buckets eight points per round trip instead of four; 41-43: the probes
  const int bpts = pe ? atoi(pe) : 4;
  const int thresh = refill_thresh(a.n);
  constexpr int SD_ = REFILL_SD<FUSE>;
  const char* fe = lab_env("TDTK_FAT_NODES");
  if (!COUNT && FUSE == 0 && thresh == 16 && bpts == 8) launch_refill<LabPts8<SD_>>(nb, lds, s, a);
  else if (!COUNT && FUSE == 0 && thresh == 16 && bpts == 41) launch_refill<LabProbe<SD_, 1>>(nb, lds, s, a);
  else if (!COUNT && FUSE == 0 && thresh == 16 && bpts == 42) launch_refill<LabProbe<SD_, 2>>(nb, lds, s, a);
  else if (!COUNT && FUSE == 0 && thresh == 16 && bpts == 43) launch_refill<LabProbe<SD_, 3>>(nb, lds, s, a);
  // two tree levels per round trip (KdFat): a measured negative, kept selectable -- see the comment at the walk
  else if (!COUNT && FUSE == 0 && thresh == 16 && a.T.fat != nullptr && fe && fe[0] == '1') launch_refill<LabFat<SD_>>(nb, lds, s, a);
  else if (thresh == 8) launch_refill<LabThresh8<COUNT, FUSE>>(nb, lds, s, a);
  else if (thresh == 16 && (FUSE == 0 || FUSE == 3) && pipe_on() && !a.skip) launch_refill<LabPipe<COUNT, (FUSE == 3 ? 3 : 0), SD_>>(nb, lds, s, a);
  else if constexpr (FUSE == 1 || FUSE == 2) {
    if (thresh == 32) launch_refill<LabFuse<32, COUNT, FUSE>>(nb, lds, s, a);
    else launch_refill<LabFuse<16, COUNT, FUSE>>(nb, lds, s, a);
  } else return false;
  return true;
}
// ---- launch_search's hook: the kernels and FUSE values that only the lab selects ----
template <bool COUNT, int FUSE> static void launch_refill128(SearchArgs& a, hipStream_t s);      // (kernels.hip, behind this file)
template <bool COUNT>
static void launch_stream128(SearchArgs& a, hipStream_t s)
{
  a.slab = stream_slab_env();
  const uint32_t nb = stream_grid(a.n);
  switch (refill_thresh(a.n)) {
    case 8: launch_refill<LabQueue<8, COUNT>>(nb, 0, s, a); break;
    case 32: launch_refill<LabQueue<32, COUNT>>(nb, 0, s, a); break;
    default: launch_refill<LabQueue<16, COUNT>>(nb, 0, s, a); break;
  }
}
template <bool COUNT, bool VOTE>
static void launch_step128(SearchArgs& a, hipStream_t s)
{
  int qpw;
  const uint32_t nb = refill_grid_b(a.n, 128, &qpw);
  a.qpw = qpw;
  switch (refill_thresh(a.n)) {
    case 8: hipLaunchKernelGGL((k_search_step<128, 4, 8, COUNT, VOTE>), dim3(nb), dim3(128), 0, s, a); break;
    case 32: hipLaunchKernelGGL((k_search_step<128, 4, 32, COUNT, VOTE>), dim3(nb), dim3(128), 0, s, a); break;
    default: hipLaunchKernelGGL((k_search_step<128, 4, 16, COUNT, VOTE>), dim3(nb), dim3(128), 0, s, a); break;
  }
}
// v: the variant launch_search has picked for the batch; g: its grid of SEARCH_BLOCK-thread workgroups.  true: *err is
// launch_search's answer.
static bool lab_launch_search(SearchArgs& a, int v, bool count, dim3 g, hipStream_t s, hipError_t* err)
{
  const dim3 b(SEARCH_BLOCK);
  *err = hipErrorInvalidValue;
  if (v == 30 && (!a.q_ctr || !a.q_ctr_next)) return true;
  const int lab_fuse = a.fuse == 2 ? 2 : ((a.fuse && a.fuse != 3) ? 1 : 0);      // (every value but 2 and the product's 3 is FUSE 1)
  if (v == 20 && lab_fuse == 2) { if (count) launch_refill128<true, 2>(a, s); else launch_refill128<false, 2>(a, s); }
  else if (v == 20 && lab_fuse == 1) { if (count) launch_refill128<true, 1>(a, s); else launch_refill128<false, 1>(a, s); }
  else if (v == 30) { if (count) launch_stream128<true>(a, s); else launch_stream128<false>(a, s); }
  else if (v == 40) { if (count) launch_step128<true, false>(a, s); else launch_step128<false, false>(a, s); }
  else if (v == 41) { if (count) launch_step128<true, true>(a, s); else launch_step128<false, true>(a, s); }
  else if (count || v == 20) return false;      // the instrumented k_search; the product's FUSE values
  else if (v == 0) hipLaunchKernelGGL((k_search<SEARCH_BLOCK, 8, false, 0, false, 1>), g, b, 0, s, a);
  else if (v == 8) {
    int qpw;
    const uint32_t nb = refill_grid_b(a.n, SEARCH_BLOCK, &qpw);
    a.qpw = qpw;
    a.phases = 1;
    launch_refill<LabBlock256>(nb, 0, s, a);
  }
  else if (v == 5) hipLaunchKernelGGL((k_search_coop<SEARCH_BLOCK, 4, 1>), g, b, 0, s, a);
  else if (v == 9) hipLaunchKernelGGL((k_search_g8<256, 16>), dim3(g8_grid(a.n)), dim3(256), 0, s, a);
  else if (v == 11) hipLaunchKernelGGL((k_search_g8<256, 16, 16>), dim3(g8_grid(a.n) * 2), dim3(256), 0, s, a);
  else if (!a.loop) return false;               // four lanes per query / one query per lane as the product launches them
  else if (v != 10 || !a.fuse) return true;     // the ICP loop without the host is the four-lanes-per-query family's alone, sums inside
  else hipLaunchKernelGGL((k_search_g8<256, 16, 4, true, true>), dim3(g8_grid4(a.n)), dim3(256), 0, s, a);
  *err = hipGetLastError();
  return true;
}
// ---- launch_search_multi's hook: single-wave workgroups, the hand-out threshold of 8, the pipelined hand-out ----
static bool lab_launch_search_multi(const SearchArgs* d_args, const uint32_t* d_base, int nbatch, uint32_t total_blocks, int thresh, bool count, bool ordered, bool lum_sums, hipStream_t s)
{
  if (!count && lum_sums && multi_block64()) {
    if (thresh == 32) launch_refill_multi<LabLinkWave<32>>(total_blocks, s, d_args, d_base, nbatch);
    else launch_refill_multi<LabLinkWave<16>>(total_blocks, s, d_args, d_base, nbatch);
  } else if (thresh == 8) {
    if (count) launch_refill_multi<LabLinkThresh8<true, false>>(total_blocks, s, d_args, d_base, nbatch);
    else if (ordered) launch_refill_multi<LabLinkThresh8<false, true>>(total_blocks, s, d_args, d_base, nbatch);
    else launch_refill_multi<LabLinkThresh8<false, false>>(total_blocks, s, d_args, d_base, nbatch);
  } else if (!count && lum_sums && pipe_on()) {
    if (thresh == 32) launch_refill_multi<LabLinkPipe<32>>(total_blocks, s, d_args, d_base, nbatch);
    else launch_refill_multi<LabLinkPipe<16>>(total_blocks, s, d_args, d_base, nbatch);
  } else return false;
  return true;
}
