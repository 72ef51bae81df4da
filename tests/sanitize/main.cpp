// tests/sanitize/main.cpp -- TEST INFRASTRUCTURE: runs the host shims (include/neighlist_cpu.hpp, include/neighlist_gpu.hpp),
// the input generator (md_neighbor_list_amd/csrc/nl_inputs.cpp) and the oracle's C restatement (oracle/nl_oracle.c) under
// AddressSanitizer + UndefinedBehaviorSanitizer on the CPU (`make asan`; tests/test_sanitizers.py).  The shims talk to
// tests/sanitize/abi_stub.cpp instead of libnl_hip.so.  And the owner of the library's device memory
// (md_neighbor_list_amd/csrc/nl_devbuf.hpp) over stand-ins of hipMalloc / hipFree: tests/sanitize/devbuf_checks.cpp.
// Exit code 0 = every check passed and no sanitizer report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "neighlist_gpu.hpp"  // defines NL_SHIM_CHECK first
#include "neighlist_cpu.hpp"

extern "C" {
int64_t nl_gen_uniform_f32(float*, int32_t, int64_t, double, double, double, uint64_t);
int64_t nl_gen_uniform_f64(double*, int32_t, int64_t, double, double, double, uint64_t);
int nl_oracle_bruteforce_f32(const float*, int32_t, int64_t, double, int, int32_t*, int64_t*, int32_t**, int64_t*);
int nl_oracle_bruteforce_f64(const double*, int32_t, int64_t, double, int, int32_t*, int64_t*, int32_t**, int64_t*);
int nl_oracle_build_f32(const float*, int32_t, int64_t, double, double, double, double, int32_t*, int64_t*, int32_t**, int64_t*);
int nl_oracle_build_pbc_f32(const float*, int32_t, int64_t, double, double, double, double, int32_t*, int64_t*, int32_t**, int64_t*);
int nl_oracle_build_pbc_full_f64(const double*, int32_t, int64_t, double, double, double, double, int32_t*, int64_t*, int32_t**, int64_t*);
int nl_oracle_count_f32(const float*, int32_t, int64_t, double, double, double, double, int32_t*, int32_t, const int32_t*, uint64_t*, int64_t*, int64_t*);
int nl_oracle_cells_f64(const double*, int32_t, int64_t, double, double, double, double, int32_t*, int32_t*);
void nl_oracle_canonicalize(int64_t, const int64_t*, int32_t*);
uint64_t nl_oracle_hash(int64_t, const int64_t*, const int32_t*);
void nl_oracle_free(void*);
}

int devbuf_checks();  // tests/sanitize/devbuf_checks.cpp: the checks that failed

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                        \
    }                                                                    \
  } while (0)

struct V3f { float x, y, z; };
struct V3d { double x, y, z; };
struct V4f { float x, y, z, w; };
struct V4d { double x, y, z, w; };

template <typename Vec, typename D> static void fill(std::vector<Vec>& q, int n, double L, uint64_t seed);
template <> void fill<V3f, float>(std::vector<V3f>& q, int n, double L, uint64_t s) { q.resize(n); nl_gen_uniform_f32(&q[0].x, 3, n, L, L, L, s); }
template <> void fill<V3d, double>(std::vector<V3d>& q, int n, double L, uint64_t s) { q.resize(n); nl_gen_uniform_f64(&q[0].x, 3, n, L, L, L, s); }
template <> void fill<V4f, float>(std::vector<V4f>& q, int n, double L, uint64_t s) { q.resize(n); nl_gen_uniform_f32(&q[0].x, 4, n, L, L, L, s); }
template <> void fill<V4d, double>(std::vector<V4d>& q, int n, double L, uint64_t s) { q.resize(n); nl_gen_uniform_f64(&q[0].x, 4, n, L, L, L, s); }

static int brute(const float* q, int stride, int n, double rc, std::vector<int32_t>& nop, std::vector<int64_t>& kp, int32_t** sl, int64_t* P) {
  return nl_oracle_bruteforce_f32(q, stride, n, rc, 0, nop.data(), kp.data(), sl, P);
}
static int brute(const double* q, int stride, int n, double rc, std::vector<int32_t>& nop, std::vector<int64_t>& kp, int32_t** sl, int64_t* P) {
  return nl_oracle_bruteforce_f64(q, stride, n, rc, 0, nop.data(), kp.data(), sl, P);
}

// the CPU class surface (make_list.cpp:148-163 flow): Initialize, MakeNeighList, accessors, against the brute force
template <typename Vec, typename D> static void cpu_class(int n, double L, double rc) {
  std::vector<Vec> q;
  fill<Vec, D>(q, n, L, 100 + n);
  NeighList<Vec> nl(rc, L, L, L);
  nl.Initialize(n);
  for (int rep = 0; rep < 2; rep++) nl.MakeNeighList(q.data(), n);
  const int stride = (int)(sizeof(Vec) / sizeof(D));
  std::vector<int32_t> nop(n + 1);
  std::vector<int64_t> kp(n + 1);
  int32_t* sl = nullptr;
  int64_t P = 0;
  CHECK(brute(&q[0].x, stride, n, rc, nop, kp, &sl, &P) == 0);
  CHECK(nl.number_of_pairs() == P);
  std::vector<int64_t> kp2(n + 1);
  for (int i = 0; i <= n; i++) kp2[i] = nl.key_pointer()[i];
  std::vector<int32_t> got(nl.sorted_list(), nl.sorted_list() + P);
  nl_oracle_canonicalize(n, kp2.data(), got.data());
  CHECK(std::equal(got.begin(), got.end(), sl));
  for (int i = 0; i < n; i++) CHECK(nl.number_of_partners()[i] == nop[i]);
  nl_oracle_free(sl);
}

// the GPU class surface (make_list.cu:113-142 flow) incl. cuda_ptr: allocate / set_val / host2dev / dev2host / operator[]
template <typename Vec, typename D> static void gpu_class(int n, double L, double rc) {
  cuda_ptr<Vec> q;
  q.allocate(n);
  std::vector<Vec> src;
  fill<Vec, D>(src, n, L, 200 + n);
  for (int i = 0; i < n; i++) q[i] = src[i];
  q.host2dev();
  cuda_ptr<int32_t> scratch;
  scratch.allocate(17);
  scratch.set_val(-1);
  scratch.set_val(3, 5, 7);
  scratch.dev2host();
  CHECK(scratch[0] == -1 && scratch[3] == 7 && scratch[7] == 7 && scratch[8] == -1 && scratch[16] == -1);
  cuda_ptr<double> d8;
  d8.allocate(5);
  d8.set_val(2.5);
  d8.dev2host(1, 3);
  CHECK(d8[1] == 2.5 && d8[3] == 2.5);
  cuda_ptr<int32_t> moved(std::move(scratch));
  CHECK(moved.size == 17 && scratch.dev_ptr == nullptr);

  NeighListGPU<Vec, D> nl((D)rc, (D)L, (D)L, (D)L);
  nl.Initialize(n);
  nl.MakeNeighList(q, n, false);
  nl.Synchronize();
  std::vector<int32_t> nop(n + 1);
  std::vector<int64_t> kp(n + 1);
  int32_t* sl = nullptr;
  int64_t P = 0;
  CHECK(brute(&src[0].x, (int)(sizeof(Vec) / sizeof(D)), n, rc, nop, kp, &sl, &P) == 0);
  CHECK(nl.number_of_pairs() == 2 * P);
  cuda_ptr<int32_t>& lst = nl.neigh_list();
  cuda_ptr<int32_t>& cnt = nl.number_of_partners();
  lst.dev2host();
  cnt.dev2host();
  int64_t up = 0, total = 0;
  for (int i = 0; i < n; i++) {
    total += cnt[i];
    for (int k = 0; k < cnt[i]; k++) {
      const int32_t j = lst[(size_t)k * n + i];
      CHECK(j >= 0 && j < n && j != i);
      if (j > i) {
        up++;
        CHECK(std::binary_search(sl + kp[i], sl + kp[i + 1], j));
      }
    }
  }
  CHECK(up == P && total == 2 * P);
  nl.UseHalfList();
  nl.MakeNeighList(q, n);
  CHECK(nl.half_number_of_pairs() == P);
  nl.key_pointer().dev2host();
  nl.sorted_list().dev2host();
  nl.half_number_of_partners().dev2host();
  CHECK(nl.key_pointer()[n] == P);
  for (int i = 0; i < n; i++) CHECK(nl.half_number_of_partners()[i] == nop[i]);
  nl_oracle_free(sl);
}

static void oracle_edges() {
  // empty input, a single particle, a particle outside the box, count mode == build mode, the minimum-image builds
  int32_t nop[8];
  int64_t kp[9];
  int32_t* sl = nullptr;
  int64_t P = -1;
  float one[4] = {1.f, 2.f, 3.f, 0.f};
  CHECK(nl_oracle_build_f32(one, 4, 0, 3.3, 12, 12, 12, nop, kp, &sl, &P) == 0 && P == 0);
  nl_oracle_free(sl);
  CHECK(nl_oracle_build_f32(one, 4, 1, 3.3, 12, 12, 12, nop, kp, &sl, &P) == 0 && P == 0 && kp[1] == 0);
  nl_oracle_free(sl);
  float far_away[4] = {100.f, 2.f, 3.f, 0.f};
  sl = nullptr;
  CHECK(nl_oracle_build_f32(far_away, 4, 1, 3.3, 12, 12, 12, nop, kp, &sl, &P) == 3);
  const int n = 3000;
  std::vector<float> q(4 * n);
  nl_gen_uniform_f32(q.data(), 4, n, 14.0, 17.0, 21.5, 5);
  std::vector<int32_t> nop1(n), nop2(n);
  std::vector<int64_t> kp1(n + 1);
  CHECK(nl_oracle_build_f32(q.data(), 4, n, 3.3, 14.0, 17.0, 21.5, nop1.data(), kp1.data(), &sl, &P) == 0);
  const uint64_t h1 = nl_oracle_hash(n, kp1.data(), sl);
  nl_oracle_free(sl);
  const int32_t slab_of_layer[6] = {0, 0, 1, 1, 2, 2};  // mesh_z = int(21.5 / 3.3) = 6
  uint64_t hs[3];
  int64_t ps[3], P2 = 0;
  CHECK(nl_oracle_count_f32(q.data(), 4, n, 3.3, 14.0, 17.0, 21.5, nop2.data(), 3, slab_of_layer, hs, ps, &P2) == 0);
  CHECK(P2 == P && ps[0] + ps[1] + ps[2] == P && hs[0] + hs[1] + hs[2] == h1 && nop1 == nop2);
  CHECK(nl_oracle_build_pbc_f32(q.data(), 4, n, 3.3, 14.0, 17.0, 21.5, nop1.data(), kp1.data(), &sl, &P2) == 0 && P2 >= P);
  nl_oracle_free(sl);
  std::vector<double> qd(q.begin(), q.end());
  CHECK(nl_oracle_build_pbc_full_f64(qd.data(), 4, n, 3.3, 14.0, 17.0, 21.5, nop1.data(), kp1.data(), &sl, &P2) == 0 && P2 >= 2 * P - 8);
  nl_oracle_free(sl);
  std::vector<int32_t> cell(n);
  int32_t mesh[3];
  CHECK(nl_oracle_cells_f64(qd.data(), 4, n, 3.3, 14.0, 17.0, 21.5, cell.data(), mesh) == 0 && mesh[0] == 4 && mesh[1] == 5 && mesh[2] == 6);
  for (int i = 0; i < n; i++) CHECK(cell[i] >= 0 && cell[i] < 120);
}

int main() {
  cpu_class<V3f, float>(1500, 14.0, 3.3);
  cpu_class<V3d, double>(1500, 14.0, 3.3);
  cpu_class<V4f, float>(700, 11.0, 2.7);
  cpu_class<V4d, double>(1, 12.0, 3.3);
  gpu_class<V4f, float>(1200, 13.0, 3.3);
  gpu_class<V4d, double>(900, 12.0, 3.0);
  oracle_edges();
  failures += devbuf_checks();
  if (failures) {
    std::fprintf(stderr, "sanitize_test: %d check(s) FAILED\n", failures);
    return 1;
  }
  std::printf("sanitize_test: all checks passed (shims, input generator, oracle restatement, device-memory owner under ASan + UBSan)\n");
  return 0;
}
