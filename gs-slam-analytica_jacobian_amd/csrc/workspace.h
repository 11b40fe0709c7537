// workspace.h -- how a caller-owned workspace is laid out (host only; DESIGN.md section 3, "How a workspace is laid out").
//
// The rules, stated once:
//   * A workspace is carved into arrays that each start on a 256-byte boundary: an array takes gsaj_align(its bytes).  The few
//     arrays that follow their predecessor unpadded (`pack`) are part of the ABI as they are and are named where they are carved.
//   * Every workspace has ONE function that takes a Carver, fills the layout struct and returns used().  The size function and
//     every entry point call that function, so a size and its layout cannot disagree.
//   * Most workspaces may be handed over at any address: the entry point starts carving at the next 256-byte boundary
//     (ALIGN_BASE), and the size function adds 256 bytes of base slack to used() to pay for that.  The batched entry points and
//     the stereo matcher refuse a workspace that is not aligned, and compaction and densification take theirs (one array of
//     32-bit words each) unaligned: these start at the pointer as given (BASE_AS_GIVEN) and their size functions add no slack.
//   * K views of a batched launch use K consecutive, identically carved blocks; a block is view_stride(bytes of one view).
//   * A Carver over a null base only measures: the pointers it hands out are never dereferenced.  Every size function carves
//     from null into a layout struct it throws away (gsaj_seed_workspace_bytes through seed_carve, and so on).
#pragma once
#include <stddef.h>
#include <stdint.h>

static inline size_t gsaj_align(size_t x) { return (x + 255) & ~(size_t)255; }
static inline char *align_base(void *p) { return reinterpret_cast<char *>(gsaj_align(reinterpret_cast<size_t>(p))); }
static inline size_t view_stride(size_t bytes) { return gsaj_align(bytes); }  // bytes between consecutive views' blocks

constexpr bool BASE_AS_GIVEN = false, ALIGN_BASE = true;  // Carver's second argument

struct Carver {  // walks a workspace; with a null base it only measures
  Carver(const void *ws, bool align) : base_(align ? gsaj_align((uintptr_t)ws) : (uintptr_t)ws), off_(0) {}
  template <typename T>
  T *take(size_t count) {  // array at the cursor; the cursor advances to the next 256-byte boundary behind it
    return at<T>(gsaj_align(sizeof(T) * count));
  }
  template <typename T>
  T *pack(size_t count) {  // the same, the next array follows unpadded
    return at<T>(sizeof(T) * count);
  }
  size_t used() const { return off_; }  // bytes from the start to the cursor

 private:
  template <typename T>
  T *at(size_t advance) {
    T *p = reinterpret_cast<T *>(base_ + off_);
    off_ += advance;
    return p;
  }
  uintptr_t base_;
  size_t off_;
};
