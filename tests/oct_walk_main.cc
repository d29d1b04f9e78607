// The octree walk of 3dtk_amd/csrc/oct_lane.h as a program of its own, for a run under -fsanitize=undefined outside Python
// (tests/test_boctree_paths_host.py builds and starts it).  It reads jobs from the file named on the command line until the
// file ends and answers each on stdout.
//
// A job:  int64 slots, points, K;  double add[3], mult, maxd2;  int32 largest_index;  uint32 top_bit;
//         uint32 nodes[slots][4];  KdPoint pts[points] (32 bytes each);  double q[K][3]
// Answer: "job <index> refused" where oct_host_find refuses the batch, else "job <index> K" and K lines
//         "<slot> <Dist2 as 16 hex digits> <leaves scanned>".
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "host_oct_shim.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv)
{
  if (argc != 2) { fprintf(stderr, "usage: %s <jobs file>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  for (int job = 0;; job++) {
    int64_t head[3];
    const size_t got = fread(head, 1, sizeof head, f);
    if (got == 0) break;
    if (got != sizeof head || head[0] < 1 || head[1] < 1 || head[2] < 0 || head[2] > INT32_MAX) { fprintf(stderr, "job %d: bad header\n", job); return 2; }
    double sc[5];
    int32_t largest;
    uint32_t top_bit;
    if (!read_all(f, sc, sizeof sc) || !read_all(f, &largest, sizeof largest) || !read_all(f, &top_bit, sizeof top_bit)) return 2;
    std::vector<OctNode> nodes((size_t)head[0]);
    std::vector<KdPoint> pts((size_t)head[1]);
    std::vector<double> q(3 * (size_t)head[2]);
    static_assert(sizeof(KdPoint) == 32, "the test writes 32-byte points");
    if (!read_all(f, nodes.data(), nodes.size() * sizeof(OctNode)) || !read_all(f, pts.data(), pts.size() * sizeof(KdPoint)) ||
        !read_all(f, q.data(), q.size() * sizeof(double))) { fprintf(stderr, "job %d: short file\n", job); return 2; }
    const int K = (int)head[2];
    std::vector<int> slot((size_t)K), leaves((size_t)K);
    std::vector<double> d2((size_t)K);
    if (oct_host_find(nodes.data(), pts.data(), sc, sc[3], largest, top_bit, q.data(), K, sc[4], slot.data(), d2.data(), leaves.data())) {
      printf("job %d refused\n", job);
      continue;
    }
    printf("job %d %d\n", job, K);
    for (int i = 0; i < K; i++) {
      uint64_t bits;
      memcpy(&bits, &d2[(size_t)i], sizeof bits);
      printf("%d %016" PRIx64 " %d\n", slot[(size_t)i], bits, leaves[(size_t)i]);
    }
  }
  fclose(f);
  return 0;
}
