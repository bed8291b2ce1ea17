// One allocation carved into the buffers of a handle: the trainer's arena and optimizer state, a model's weight blob, a session's
// workspace.
#pragma once

#include "common.h"

#include <functional>
#include <vector>

namespace m2m {

// Sizes one device allocation and points the members at their parts of it.  A buffer is declared ONCE, as take(member, bytes): it
// gets the next 256-byte aligned offset, and the carver notes (member, offset); bind(base), after the allocation, sets every noted
// member to base + offset.  The order of the declarations is the layout.  The carver keeps REFERENCES to the members: a container of
// them (the per-layer structs, the residual streams, the rings) is resized before the first declaration into it and never grows after.
struct Carver {
  int64_t off = 0;
  std::vector<std::function<void(unsigned char*)>> binds;
  int64_t take(int64_t bytes) { const int64_t o = off; off = align_up(off + bytes, 256); return o; }      // unnamed: a reservation
  template <typename P>
  void take(P*& member, int64_t bytes) {
    const int64_t o = take(bytes);
    binds.push_back([&member, o](unsigned char* base) { member = reinterpret_cast<P*>(base + o); });
  }
  void bind(unsigned char* base) const { for (const auto& b : binds) b(base); }
};

}  // namespace m2m
