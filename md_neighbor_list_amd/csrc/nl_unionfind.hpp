// nl_unionfind.hpp -- the lock-free union-find behind nl_clusters (nl_cluster.inc): find with path
// halving and unite by minimum-hooking on an int32 parent array, written against an atomics policy A with
//   A::load(p)            an atomic load of *p,
//   A::store(p, v)        an atomic store,
//   A::cas(p, want, v)    *p = v iff *p == want, atomically; returns what *p held.
// UfDevice (HIP builtins, relaxed, agent scope) is the policy of the kernels; UfHost (__atomic_*, relaxed) lets a host program
// run the same two functions under std::thread (tests/tsan/unionfind_check.cpp, `make tsan`).  Nothing here orders anything:
// union-find needs every access to be atomic and the invariant below, not an order between accesses.
//
// The invariant: parent[v] <= v at every moment, with equality only at a root; and parent[v] is a vertex of v's own tree.
//   - parent[v] = v at the start.
//   - A hook writes parent[big] = small < big, by a CAS that succeeds only while big is still a root: a vertex that has a
//     parent never becomes a root again, and every root loses that state at most once.
//   - A halving store writes parent[v] = g where g was read as parent[parent[v]]: a vertex of the same tree, g < v.  A store
//     that arrives late (another thread has meanwhile written a lower one) puts back an older value, which is still a vertex
//     of the same tree below v: paths grow longer again, nothing else.
// So whatever stale value a load returns, a find walks strictly decreasing indices and ends after at most v steps by its own
// progress; it waits for nobody.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define NL_UF_FN __host__ __device__ __forceinline__
#else
#define NL_UF_FN inline
#endif

namespace nl {

#if defined(__HIPCC__)
// Relaxed atomics at agent scope: the loads bypass the CU's L1 (which another CU's stores never refresh) and the stores and
// the CAS are performed in the memory that all XCDs share, not left in one XCD's L2.
struct UfDevice {
  static __device__ __forceinline__ int32_t load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ void store(int32_t* p, int32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ int32_t cas(int32_t* p, int32_t want, int32_t v) {
    __hip_atomic_compare_exchange_strong(p, &want, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return want;  // (what *p held: `want` itself where the exchange took place)
  }
};
#endif

struct UfHost {
  static int32_t load(const int32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
  static void store(int32_t* p, int32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
  static int32_t cas(int32_t* p, int32_t want, int32_t v) {
    __atomic_compare_exchange_n(p, &want, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return want;
  }
};

// The root of v's tree as of some moment during the call.  Halves the path on its way: parent[v] = parent[parent[v]].
// Ends by its own progress: every step goes to a strictly smaller index (the invariant), so at most v steps.
template <typename A> NL_UF_FN int32_t uf_find(int32_t* parent, int32_t v) {
  for (;;) {
    const int32_t p = A::load(parent + v);
    if (p == v) return v;
    const int32_t g = A::load(parent + p);
    if (g == p) return p;
    A::store(parent + v, g);  // (g < p < v, a vertex of the same tree)
    v = g;
  }
}

// The same without a store: for the pass that turns the parent array into the labels in place (k_cc_flatten), where an entry
// that its own thread has set to its root must not be put back to an older ancestor by another thread's late halving store.
template <typename A> NL_UF_FN int32_t uf_root(const int32_t* parent, int32_t v) {
  for (;;) {
    const int32_t p = A::load(parent + v);
    if (p == v) return v;
    v = p;
  }
}

// The trees of a and b become one.  The LARGER root goes under the smaller, so the root of a finished component is its
// smallest index whatever the schedule.  A CAS that fails means that another thread took the root state from `big` in the
// meantime -- which happens to every vertex at most once, n times in all -- and the loop goes on from the new roots: from the
// parent the CAS itself returned for `big` (below big, so this side has moved down even if every load were stale) and from
// `small`.  No thread waits for a value another has yet to write.
template <typename A> NL_UF_FN void uf_unite(int32_t* parent, int32_t a, int32_t b) {
  for (;;) {
    a = uf_find<A>(parent, a);
    b = uf_find<A>(parent, b);
    if (a == b) return;
    const int32_t big = a > b ? a : b, small = a > b ? b : a;
    const int32_t was = A::cas(parent + big, big, small);
    if (was == big) return;
    a = was, b = small;
  }
}

}  // namespace nl
