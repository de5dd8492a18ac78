// Who owns what the host side of the library allocates on the device (plain C++: tests/host_layout_check.cpp builds it
// with g++ and an allocator of its own).
//
// DevOwner records every block at allocation time and frees what it still holds exactly once, in free_all() or when it
// goes out of scope.  The handle keeps one for its life (monsoon_destroy walks it); a call that needs temporaries keeps
// one on its stack, so every return path frees them.  DevBuffers and the other structs that travel to kernels keep the
// raw pointers the owner hands out.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <vector>

// The allocator: 0 = success, anything else is the runtime's error code.  A program that defines HOST_MEM_ALLOCATOR
// before including this header supplies the two functions itself.
#ifndef HOST_MEM_ALLOCATOR
#include <hip/hip_runtime.h>
inline int host_mem_alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
inline int host_mem_free(void* p) { return (int)hipFree(p); }
#endif

// Replace: free, then allocate; on failure the pointer is null and the capacity 0.
// Retire: allocate, then keep the old block until free_all(); work already recorded may still point to it.
enum class Grow { Replace, Retire };

// (Hidden visibility here and on LazyObjects: host helpers of one translation unit stay out of a library's exported symbols.)
struct __attribute__((visibility("hidden"))) DevOwner {
  std::vector<void*> blocks;   // every block this owner has to free, live or retired

  DevOwner() = default;
  DevOwner(const DevOwner&) = delete;
  DevOwner& operator=(const DevOwner&) = delete;
  ~DevOwner() { free_all(); }

  template <class T>
  int alloc(T** p, size_t bytes) {
    blocks.reserve(blocks.size() + 1);   // (the record cannot fail once the block exists)
    void* q = nullptr;
    const int e = host_mem_alloc(&q, bytes);
    if (e) return e;
    blocks.push_back(q);
    *p = (T*)q;
    return 0;
  }
  // Room for `want` units (`bytes` in all) where `cap` units are there: nothing to do if they suffice.
  template <class T, class N>
  int grow(T*& p, N& cap, N want, size_t bytes, Grow policy) {
    if (want <= cap) return 0;
    auto old = std::find(blocks.begin(), blocks.end(), (void*)p);
    if (policy == Grow::Replace && old != blocks.end()) {
      blocks.erase(old);
      host_mem_free(p);
      p = nullptr;
      cap = 0;
    }
    const int e = alloc(&p, bytes);
    if (!e) cap = want;
    return e;
  }
  // What a call prepared in an owner of its own and the handle keeps from now on.
  void adopt(DevOwner& from) {
    for (void* p : from.blocks) blocks.push_back(p);
    from.blocks.clear();
  }
  void free_all() {
    for (void* p : blocks) host_mem_free(p);
    blocks.clear();
  }
};

// The trivially small sibling for events and streams: created on first use through `make` (0 = success), destroyed once.
template <class T>
struct __attribute__((visibility("hidden"))) LazyObjects {
  std::vector<T> all;
  template <class Make>
  int get(T& slot, Make make) {
    if (slot) return 0;
    const int e = (int)make(&slot);
    if (!e) all.push_back(slot);
    return e;
  }
  template <class Destroy>
  void destroy_all(Destroy destroy) {
    for (T x : all) destroy(x);
    all.clear();
  }
};
