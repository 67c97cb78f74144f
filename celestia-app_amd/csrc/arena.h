// arena.h — carving one device buffer into consecutive 256-byte-aligned slots.  Plain C++ (no HIP header): the proof
// calls' staging (sampling.cpp, befp.cpp) and their workspace layouts (sampling.h) walk an Arena, and so does
// tests/san/arena_check.cpp under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cda {

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// A walk over a buffer whose base is 256-byte aligned.  With a null base the walk only measures: every take returns
// null and used() is what the same walk needs of a real buffer.  A take of nothing is legal and returns the current
// position without moving it (the kernels are handed such pointers for sections a call leaves empty).
struct Arena {
  uint8_t* base = nullptr;
  size_t off = 0;  // always a multiple of 256
  Arena() = default;
  explicit Arena(void* p) : base((uint8_t*)p) {}
  template <class T>
  T* take(size_t count) {
    T* at = base ? (T*)(base + off) : nullptr;
    off += align256(count * sizeof(T));
    return at;
  }
  size_t used() const { return off; }
};

}  // namespace cda
