// scratch_layout.h -- the regions of one host-array call inside the context's scratch buffer (ScratchCall, okvfe_ctx.h).
// Plain C++, nothing of HIP: tests/cpp/scratch_layout_main.cpp compiles it on the host.
#pragma once
#include <cstddef>

namespace okvfe {

// Every region starts at a multiple of 256 bytes and holds at least one byte, so an empty array still has an address of
// its own.  Where a region lies is nobody's contract; that it is aligned and distinct is.
class ScratchLayout {
 public:
  size_t take(size_t bytes) {
    const size_t o = total_;
    total_ = (total_ + (bytes ? bytes : 1) + 255) / 256 * 256;
    return o;
  }
  size_t total() const { return total_; }

 private:
  size_t total_ = 0;
};

}  // namespace okvfe
