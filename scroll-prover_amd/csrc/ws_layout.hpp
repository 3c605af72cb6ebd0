// ws_layout.hpp -- where the fields of one workspace block go: a bump allocator over byte offsets.  Plain C++, no HIP: the entry points that keep several arrays in ONE pooled
// mi355_buf block (lib_aux.hip, lib_pairing.hip) name each field once, in order, and ask total() for the size of the block, instead of adding offsets up by hand; the same code
// runs under the host-side check tests/hostcheck/ws_layout_main.cpp.
//
// take(bytes) hands out the current offset and advances by `bytes` rounded up to 256 -- the granularity of mi355_buf_alloc, so a block laid out by take() alone starts every field
// on a 256-byte line.  take_exact(bytes) advances by `bytes` as they are: for arrays of one element type packed back to back.  A field of 0 bytes takes no room.
#pragma once
#include <cstdint>

namespace mi355zk {

struct WsLayout {
  uint64_t end = 0;
  uint64_t take(uint64_t bytes) { return take_exact((bytes + 255) & ~255ull); }
  uint64_t take_exact(uint64_t bytes) { const uint64_t off = end; end += bytes; return off; }
  uint64_t total() const { return end; }
};

}  // namespace mi355zk
