// tests/sanitize/devbuf_checks.cpp -- TEST INFRASTRUCTURE: the owner of the library's device memory
// (md_neighbor_list_amd/csrc/nl_devbuf.hpp) compiled by the host compiler against stand-ins of hipMalloc / hipFree over
// malloc / free, and driven through every operation the library uses, under ASan + UBSan + LSan (`make asan`; called from
// tests/sanitize/main.cpp).  No device, no HIP runtime: a leak, a double free or a use after free is the sanitizers' to
// report, the sizes and the pointers that survive a failure are checked here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "nl_devbuf.hpp"

namespace {
long live = 0;         // stand-in allocations not yet freed
long allocs = 0;       // stand-in allocations made
long fail_at = -1;     // the allocation (counted from 0) that fails; -1: none
size_t last_bytes = 0;  // bytes the last successful allocation was asked for
}  // namespace

extern "C" hipError_t hipMalloc(void** p, size_t bytes) {
  if (allocs++ == fail_at) {
    *p = nullptr;
    return hipErrorOutOfMemory;
  }
  *p = std::malloc(bytes);  // (exactly what was asked for: ASan then catches a write past a 16-byte minimum)
  if (!*p) return hipErrorOutOfMemory;
  std::memset(*p, 0xA5, bytes);
  last_bytes = bytes;
  live++;
  return hipSuccess;
}
extern "C" hipError_t hipFree(void* p) {
  if (p) live--;
  std::free(p);  // (a second free of the same pointer is ASan's to report)
  return hipSuccess;
}

namespace {
int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                        \
    }                                                                    \
  } while (0)

void fail_next() { fail_at = allocs; }

struct Several {  // a handle in small: members freed by the implicit destructor, an empty one among them
  nl::DevBuf<int32_t> a, b;
  nl::DevBuf<void> c, never;
  nl::DevBuf<uint64_t> arr[2];
};

void takes_raw(const int32_t* p, void* q) { CHECK(p != nullptr && q != nullptr); }
}  // namespace

int devbuf_checks() {
  using nl::DevBuf;
  {  // empty: converts to null, holds nothing (not even zero items), releases any number of times
    DevBuf<int32_t> e;
    CHECK(!e && e.get() == nullptr && e.bytes() == 0 && e.items() == 0 && !e.holds(0));
    e.release();
    e.release();
  }
  {  // replace: frees the old allocation first; empty after a failure
    DevBuf<int32_t> b;
    CHECK(b.replace(400, 100) == hipSuccess && b && b.bytes() == 400 && b.items() == 100 && b.holds(100) && !b.holds(101));
    b.get()[99] = 7;
    int32_t* const first = b;
    CHECK(first + 99 == b + 99 && *(b + 99) == 7);  // (pointer arithmetic as on a raw pointer)
    CHECK(live == 1);
    CHECK(b.replace(800, 200) == hipSuccess && b.items() == 200 && live == 1);
    b.get()[199] = 9;
    fail_next();
    CHECK(b.replace(1600, 400) == hipErrorOutOfMemory);
    CHECK(!b && b.bytes() == 0 && b.items() == 0 && !b.holds(0) && live == 0);
    b.release();  // (released twice: by the failure and here)
  }
  {  // zero bytes: 16 are allocated, zero are reported
    DevBuf<void> z;
    CHECK(z.replace(0) == hipSuccess && z && last_bytes == 16 && z.bytes() == 0 && z.holds(0));
    std::memset(z, 0, 16);
  }
  {  // replace, keeping the old allocation where the new one cannot be had
    DevBuf<uint64_t> k;
    CHECK(k.replace_keeping(80, 10) == hipSuccess && k.items() == 10);  // (onto an empty buffer)
    uint64_t* const old = k;
    old[9] = 42;
    fail_next();
    CHECK(k.replace_keeping(160, 20) == hipErrorOutOfMemory);
    CHECK(k.get() == old && k.bytes() == 80 && k.items() == 10 && k[9] == 42 && live == 1);
    CHECK(k.replace_keeping(160, 20) == hipSuccess && k.bytes() == 160 && k.items() == 20 && live == 1);
    k.get()[19] = 1;
  }
  {  // ensure: grows, does not shrink or reallocate where it holds enough, holds nothing after a failed growth
    DevBuf<int32_t> g;
    CHECK(g.ensure(0, 64) == hipSuccess && g && g.holds(0));  // (an empty buffer does not hold zero items: it allocates)
    CHECK(g.ensure(10, 40) == hipSuccess && g.items() == 10 && g.bytes() == 40);
    int32_t* const p10 = g;
    const long before = allocs;
    CHECK(g.ensure(10, 40) == hipSuccess && g.ensure(3, 12) == hipSuccess && g.get() == p10 && g.items() == 10 && allocs == before);
    CHECK(g.ensure(11, 44) == hipSuccess && g.items() == 11 && allocs == before + 1 && live == 1);
    g.get()[10] = 5;
    fail_next();
    CHECK(g.ensure(12, 48) == hipErrorOutOfMemory && !g && !g.holds(0) && g.items() == 0 && live == 0);
    CHECK(g.ensure(12, 48) == hipSuccess && g.holds(12));  // (and the next call tries again)
  }
  {  // sized by n_max on first use and re-checked with holds() by every later use, released when the handle is initialised
    // again (the counts and cursors of nl_get_full_transposed): taken for n_max = 300, it never serves n_max = 6000
    DevBuf<int32_t> t;
    auto first_use = [&t](int64_t n_max) { return t.ensure(n_max, 4 * ((size_t)n_max + 16)); };
    CHECK(first_use(300) == hipSuccess && t.items() == 300 && t.bytes() == 4 * 316);
    t.get()[315] = 1;
    CHECK(!t.holds(6000));  // (with or without the release in between)
    CHECK(first_use(6000) == hipSuccess && t.items() == 6000 && t.bytes() == 4 * 6016 && live == 1);
    t.get()[5999] = 1;  // (what the kernels write for a build of 6000: inside, or ASan reports it)
    t.release();  // nl_initialize
    CHECK(!t.holds(0) && live == 0);
    CHECK(first_use(300) == hipSuccess && t.bytes() == 4 * 316 && live == 1);  // (a handle made smaller: a small one again)
  }
  {  // move-assignment onto a buffer that holds something; move construction; self-adoption
    DevBuf<int32_t> a, b;
    CHECK(a.replace(40, 10) == hipSuccess && b.replace(80, 20) == hipSuccess && live == 2);
    int32_t* const pb = b;
    a = std::move(b);
    CHECK(a.get() == pb && a.items() == 20 && a.bytes() == 80 && !b && b.items() == 0 && live == 1);
    DevBuf<int32_t> c(std::move(a));
    CHECK(c.get() == pb && !a && live == 1);
    c.adopt(c);
    CHECK(c.get() == pb && c.items() == 20 && live == 1);
    // adopt: the table hand-over of the exclusion set-up (a scratch buffer becomes the handle's, the old table goes)
    DevBuf<int32_t> table, scratch;
    CHECK(table.replace(16, 4) == hipSuccess && scratch.replace(32, 8) == hipSuccess && live == 3);
    int32_t* const ps = scratch;
    table.adopt(scratch);
    CHECK(table.get() == ps && table.items() == 8 && table.bytes() == 32 && !scratch && scratch.bytes() == 0 && live == 2);
    table.adopt(scratch);  // (adopting an empty buffer releases)
    CHECK(!table && live == 1);
  }
  {  // conversions: to its own pointer type implicitly, from void to any pointer by static_cast
    DevBuf<int32_t> i;
    DevBuf<void> v;
    CHECK(i.replace(8) == hipSuccess && v.replace(8) == hipSuccess);
    takes_raw(i, v);
    takes_raw(static_cast<const int32_t*>(v), i);
    CHECK(static_cast<float*>(v) == v.get());
  }
  {  // a struct of several: every member freed once by the implicit destructor, an early return included
    auto early = [](bool leave) -> int {
      Several s;
      if (s.a.replace(4) != hipSuccess || s.b.replace(4) != hipSuccess || s.c.replace(4) != hipSuccess) return 1;
      if (leave) return 2;
      if (s.arr[0].replace(8) != hipSuccess || s.arr[1].replace(8) != hipSuccess) return 1;
      s.b.release();
      return 0;
    };
    CHECK(early(true) == 2 && live == 0);
    CHECK(early(false) == 0 && live == 0);
    Several* heap = new Several();  // (as the handle: new, members filled, delete)
    CHECK(heap->a.replace(4) == hipSuccess && heap->arr[1].replace(4) == hipSuccess && live == 2);
    delete heap;
  }
  CHECK(live == 0);
  return failures;
}
