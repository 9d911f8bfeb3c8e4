// sls_arena.h — the one arena type: a device allocation declared as a list of tables to upload and buffers the owner keeps,
// and the arithmetic that lays the list out (plain C++, no HIP: tests/host_sanitize drives it).  The commit functions, which
// issue the HIP calls for a layout, are in sls_object.hip.  Plans, the objects that evaluate a resident Φ and the device
// symbolic routes all keep their device memory in one of these.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

struct sls_ctx;
struct ihipStream_t;

namespace sls {

class Arena {
 public:
  // the room a block of b bytes takes: at least 16 bytes, rounded up to 256
  static size_t al(size_t b) { return (std::max<size_t>(b, 16) + 255) / 256 * 256; }
  static constexpr size_t kStageAll = SIZE_MAX;         // lay_out: every table is staged
  static constexpr size_t kClearUpTo = 1u << 20;        // clear: buffers of at most this many bytes
  // a table to upload; *out is its device copy after commit
  template <class V>
  void table(const V& v, const typename V::value_type** out) {
    add(v.empty() ? nullptr : v.data(), v.size() * sizeof(typename V::value_type), reinterpret_cast<const void**>(out), false);
  }
  // n elements the owner keeps, uninitialised; *out after commit
  template <class T>
  void buffer(size_t n, T** out) { add(nullptr, n * sizeof(T), reinterpret_cast<const void**>(const_cast<const T**>(out)), true); }
  // bytes declared so far, each block with its room: the size of the arena, and for `commit` the offset of the next declaration
  size_t bytes() const { return total_; }

  // Where commit_in puts every declaration.  Tables of at most `in_place_above` bytes come first: they are staged on the host
  // and go up in ONE copy of [0, staged_end).  Larger tables follow, each copied in place from the caller's memory; buffers
  // come last.  The order of the declarations is kept within each of the three.  An empty table has nothing to upload and
  // ranks with the buffers; like every block it gets an address of its own.
  struct Layout {
    std::vector<size_t> off;            // by declaration
    size_t total = 0, staged_end = 0;
    // what `clear` zeroes: the buffers of at most kClearUpTo bytes, whose hull is [clear_begin, clear_end) — empty when there is
    // none.  clear_hull: no larger buffer lies inside the hull, so one memset over it does; otherwise one per buffer.
    size_t clear_begin = 0, clear_end = 0;
    bool clear_hull = true;
  };
  Layout lay_out(size_t in_place_above = kStageAll) const {
    auto rank = [&](const Req& r) { return r.src == nullptr ? 2 : (r.bytes <= in_place_above ? 0 : 1); };
    Layout L;
    L.off.resize(reqs_.size());
    for (int k = 0; k < 3; ++k)
      for (size_t i = 0; i < reqs_.size(); ++i) {
        if (rank(reqs_[i]) != k) continue;
        L.off[i] = L.total;
        L.total += al(reqs_[i].bytes);
        if (k == 0) L.staged_end = L.total;
      }
    auto cleared = [&](const Req& r) { return r.own && r.bytes <= kClearUpTo; };
    L.clear_begin = L.total;
    for (size_t i = 0; i < reqs_.size(); ++i)
      if (cleared(reqs_[i])) { L.clear_begin = std::min(L.clear_begin, L.off[i]); L.clear_end = std::max(L.clear_end, L.off[i] + reqs_[i].bytes); }
    if (L.clear_end <= L.clear_begin) L.clear_begin = L.clear_end = 0;
    for (size_t i = 0; i < reqs_.size(); ++i)
      if (reqs_[i].own && !cleared(reqs_[i]) && L.off[i] >= L.clear_begin && L.off[i] < L.clear_end) L.clear_hull = false;
    return L;
  }
  // hipMalloc on the current device, the tables one synchronous copy each, the pointers; the blocks lie in the order of the
  // declarations.  On a failure nothing stays allocated, *arena is NULL and the result is hipfail's, with `what_malloc` or
  // `what_upload`.
  int commit(sls_ctx* ctx, void** arena, const char* what_malloc, const char* what_upload);
  // `lay` inside lay.total bytes of device memory the caller owns: the staged tables through `stage` (lay.staged_end bytes the
  // caller supplies, pinned if it has them; NULL: a host vector) in ONE synchronous copy, the others in place, the pointers.  A
  // failure is hipfail's with `what_upload`.  The short form stages every table.
  int commit_in(sls_ctx* ctx, void* base, const Layout& lay, unsigned char* stage, const char* what_upload);
  int commit_in(sls_ctx* ctx, void* base, const char* what_upload) { return commit_in(ctx, base, lay_out(), nullptr, what_upload); }
  // zeroes what `lay` says is cleared, on `stream`; a failure is hipfail's with `what`
  int clear(sls_ctx* ctx, void* base, const Layout& lay, ihipStream_t* stream, const char* what) const;

 private:
  struct Req { const void* src; size_t bytes; const void** out; bool own; };   // own: a buffer (an empty table has no src either)
  void add(const void* src, size_t bytes, const void** out, bool own) { reqs_.push_back({src, bytes, out, own}); total_ += al(bytes); }
  std::vector<Req> reqs_;
  size_t total_ = 0;
};

}  // namespace sls
