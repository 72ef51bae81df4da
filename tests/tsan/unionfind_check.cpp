// unionfind_check.cpp -- the union-find of nl_clusters (md_neighbor_list_amd/csrc/nl_unionfind.hpp) with the host atomics
// policy under 16 std::threads, compared against a serial union-find.  Built by `make tsan` with -fsanitize=thread: every access
// to the parent array must be an atomic, and the result must be the smallest index of every component whatever the schedule.
// The graphs: random ones below and above their percolation threshold, a path whose edges come in shuffled order (the
// longest paths a find can meet), a star (every unite meets at one root) and a clique (every CAS contends).
// Each thread takes the edges e with e % 16 == its number; after the join the parent array is turned into the labels in place by
// uf_root, as k_cc_flatten does it, again from 16 threads, and the array itself is compared.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#include "nl_unionfind.hpp"

namespace {

constexpr int THREADS = 16;
using Edges = std::vector<std::pair<int32_t, int32_t>>;

// The canonical labels by a serial union-find of its own (no code shared with the header): the smallest index of a component.
std::vector<int32_t> serial_labels(int32_t n, const Edges& edges) {
  std::vector<int32_t> p(n);
  std::iota(p.begin(), p.end(), 0);
  auto find = [&](int32_t v) {
    while (p[v] != v) v = p[v];
    return v;
  };
  for (const auto& e : edges) {
    const int32_t a = find(e.first), b = find(e.second);
    if (a != b) p[std::max(a, b)] = std::min(a, b);
  }
  std::vector<int32_t> out(n);
  for (int32_t v = 0; v < n; v++) out[v] = find(v);
  return out;
}

std::vector<int32_t> threaded_labels(int32_t n, const Edges& edges) {
  std::vector<int32_t> p(n);
  std::iota(p.begin(), p.end(), 0);
  std::vector<std::thread> pool;
  for (int t = 0; t < THREADS; t++)
    pool.emplace_back([&, t] {
      for (size_t e = t; e < edges.size(); e += THREADS) nl::uf_unite<nl::UfHost>(p.data(), edges[e].first, edges[e].second);
    });
  for (auto& th : pool) th.join();
  pool.clear();
  for (int32_t v = 0; v < n; v++)
    if (p[v] > v) return {-1};  // the invariant
  // the labels in place, as k_cc_flatten writes them: every entry by its own thread, while the others still walk the array
  for (int t = 0; t < THREADS; t++)
    pool.emplace_back([&, t] {
      for (int32_t v = t; v < n; v += THREADS) {
        const int32_t r = nl::uf_root<nl::UfHost>(p.data(), v);
        if (r != v) nl::UfHost::store(p.data() + v, r);
      }
    });
  for (auto& th : pool) th.join();
  return p;
}

int check(const char* name, int32_t n, const Edges& edges) {
  const std::vector<int32_t> want = serial_labels(n, edges);
  for (int rep = 0; rep < 3; rep++) {
    if (threaded_labels(n, edges) != want) {
      std::printf("FAIL %s: n = %d, %zu edges, repeat %d\n", name, n, edges.size(), rep);
      return 1;
    }
  }
  int32_t comps = 0;
  for (int32_t v = 0; v < n; v++) comps += want[v] == v;
  std::printf("ok   %s: n = %d, %zu edges, %d components\n", name, n, edges.size(), comps);
  return 0;
}

}  // namespace

int main() {
  std::mt19937 rng(12345);
  int bad = 0;
  for (const double deg : {0.5, 0.9, 1.2, 4.0}) {  // mean degree: below, near and above the giant component's threshold at 1
    const int32_t n = 20000;
    Edges e((size_t)(deg * n / 2));
    std::uniform_int_distribution<int32_t> pick(0, n - 1);
    for (auto& p : e) p = {pick(rng), pick(rng)};  // (self loops and duplicates included)
    char name[64];
    std::snprintf(name, sizeof name, "random graph, mean degree %.1f", deg);
    bad += check(name, n, e);
  }
  {
    const int32_t n = 30000;  // a path through shuffled indices, its edges in shuffled order
    std::vector<int32_t> id(n);
    std::iota(id.begin(), id.end(), 0);
    std::shuffle(id.begin(), id.end(), rng);
    Edges e;
    for (int32_t k = 0; k + 1 < n; k++) e.push_back({id[k], id[k + 1]});
    std::shuffle(e.begin(), e.end(), rng);
    bad += check("path, shuffled", n, e);
  }
  {
    const int32_t n = 30000, hub = 17321;
    Edges e;
    for (int32_t v = 0; v < n; v++) e.push_back({hub, v});
    std::shuffle(e.begin(), e.end(), rng);
    bad += check("star", n, e);
  }
  {
    const int32_t n = 300;
    Edges e;
    for (int32_t a = 0; a < n; a++)
      for (int32_t b = a + 1; b < n; b++) e.push_back({b, a});
    std::shuffle(e.begin(), e.end(), rng);
    bad += check("clique", n, e);
  }
  {
    Edges e;  // isolated vertices and an empty graph
    bad += check("no edges", 1000, e);
    bad += check("no vertices", 0, e);
  }
  std::printf("unionfind_check: %d failed\n", bad);
  return bad ? 1 : 0;
}
