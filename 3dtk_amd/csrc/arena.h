// Carving a scratch arena into named, typed regions: the two tree builders (build.hip, ann.hip).
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace tdtk {

// where a region starts, and what lives there
template <class T>
struct Region {
  size_t off = 0;
  T* in(char* arena) const { return static_cast<T*>(static_cast<void*>(arena + off)); }
};

// Lab library: every region of an arena is followed by 256 guard bytes, filled with a pattern before a build and looked
// at behind it -- a region written past its end (the hand-over bug of round 4: a million root records into a table of
// 8192) fails the build it happens in, whatever it would have hit.  The product's layout has no guards.
#ifdef TDTK_LAB
constexpr size_t ARENA_GUARD = 256;
#else
constexpr size_t ARENA_GUARD = 0;
#endif
constexpr uint32_t ARENA_GUARDS_MAX = 250;
struct GuardList { uint32_t n; uint32_t pad; size_t off[ARENA_GUARDS_MAX]; };

// The one place that knows how regions follow each other: each starts where the last one ended, takes its bytes rounded
// up to 256 and (lab) a guard, whose offset is noted.
struct ArenaCarver {
  size_t off = 0;
  GuardList guards{};
  template <class T>
  void take(Region<T>& r, size_t bytes)
  {
    r.off = off;
    off += (bytes + 255) & ~(size_t)255;
    if (ARENA_GUARD) {
      if (guards.n < ARENA_GUARDS_MAX) guards.off[guards.n++] = off;
      off += ARENA_GUARD;
    }
  }
};

// arm before the build, check after it (build.hip; nothing in the product).  The check returns 0, or 1 + the index of an
// overwritten guard; `d_bad` is a device word of the arena that nothing else uses.
void arena_guards_arm(char* arena, const GuardList& G, hipStream_t s);
uint32_t arena_guards_check(char* arena, const GuardList& G, uint32_t* d_bad, hipStream_t s);

}  // namespace tdtk
