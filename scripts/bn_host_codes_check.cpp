// Host-only comparison of two builds of libhfpcg.so: the return codes of the BatchNorm / affine entry points of
// hf_bn.hip whose validators take the public problem structs (hf_chan_affine[_ex|_pair], hf_chan_affine_train[_pair],
// hf_chan_affine_bwd[_ex|_pair], hf_bn_adjoint_v4[_pair]) on the same seeded random argument sets.  A set is a valid
// base problem with 0, 1 or 2 of its fields changed to a value that may be a fault (a null or misaligned pointer, a size
// of 0 / -1 / no multiple of 4 / beyond a limit, a bad split count, slab stride, leading dimension, row-block count,
// dtype ...).  Pointers are fake and never dereferenced: a set both builds accept reaches the launch and comes back with
// the runtime's no-device error, so this program runs ONLY where there is no GPU and stops if it finds one.
//
//   c++ -std=c++17 -Iinclude -fsanitize=address,undefined scripts/bn_host_codes_check.cpp -ldl -o bn_host_codes_check
//   ./bn_host_codes_check <old libhfpcg.so> <new libhfpcg.so> [sets per entry point]
//
// Exit status 0: every set with at most one changed field returns the same code from both; differences among the sets
// with two changed fields are counted and printed.
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>
#include <vector>

#include "hf_pcg.h"

static std::mt19937_64 rng(20240611);
static int rnd(int n) { return (int)(rng() % (uint64_t)n); }
template <typename T>
static T pick(std::initializer_list<T> v) { return v.begin()[rnd((int)v.size())]; }
static void* fake(int k) { return (void*)(uintptr_t)(0x100000 + 0x1000 * k); }

template <typename P>
static void bad_ptr(P& p) { p = (rnd(2) || !p) ? (P) nullptr : (P)((const char*)p + pick({4, 8})); }
static void bad_size(int64_t& v) { v = pick<int64_t>({0, -1, 3, 6, 4100, 1 << 20, 1LL << 31}); }
static void bad_splits(int& v) { v = pick({0, -1, 1, 2, 3, 33}); }
static void bad_slab(int64_t& v) { v = pick<int64_t>({0, -4, 6, 144, 1 << 20}); }
static void bad_ld(int64_t& v) { v = pick<int64_t>({0, 1, 6, 10, 32, 0x40000000LL}); }
static void bad_dtype(int& v) { v = pick({(int)HF_F64, 7, -1}); }

struct Aff { hf_affine_problem p; int cl, dtype; };
struct Train { hf_affine_train_problem p; int64_t add_ld; int dtype; };
struct Adj { hf_bn_adjoint_problem p; int cl, dtype; };

static Aff base_aff() {
  Aff s{};
  s.p = {fake(0), fake(1), fake(2), fake(3), fake(4), fake(5), fake(6), fake(7), fake(8), fake(9), rnd(2),
         2, 8, 9, 16, 16, 2, 144};
  if (rnd(3) == 0) s.p.c = 6, s.p.out_ld = s.p.add_ld = 12;  // (the scalar walk)
  s.cl = 1, s.dtype = rnd(4) ? HF_F32 : HF_F64;
  return s;
}
static Train base_train() {
  Train s{};
  s.p = {fake(0), fake(1), fake(2), fake(3), fake(4), fake(5), fake(6), fake(7), 3, fake(8), fake(9), 18.0, fake(10),
         fake(11), 2, 8, 9, 16, 2, 144};
  s.add_ld = 16, s.dtype = HF_F32;
  return s;
}
static Adj base_adj() {
  Adj s{};
  s.p = {fake(0), fake(1), fake(2), fake(3), fake(4), 2, 144, fake(5), 2, 144, fake(6), fake(7), fake(8), fake(9),
         fake(10), 2, 8, 9, pick({1, 3})};
  s.cl = 1, s.dtype = HF_F32;
  return s;
}

typedef std::function<void(Aff&)> AffM;
typedef std::function<void(Train&)> TrainM;
typedef std::function<void(Adj&)> AdjM;
#define M(T, body) [](T& s) { body; }
static const std::vector<AffM> aff_changes = {
    M(Aff, bad_ptr(s.p.out)), M(Aff, bad_ptr(s.p.a)), M(Aff, bad_ptr(s.p.x)), M(Aff, bad_ptr(s.p.mean)),
    M(Aff, bad_ptr(s.p.rstd)), M(Aff, bad_ptr(s.p.w)), M(Aff, bad_ptr(s.p.q)), M(Aff, bad_ptr(s.p.r)),
    M(Aff, bad_ptr(s.p.add)), M(Aff, bad_ptr(s.p.mask_src)), M(Aff, bad_size(s.p.n)), M(Aff, bad_size(s.p.c)),
    M(Aff, bad_size(s.p.hw)), M(Aff, bad_ld(s.p.out_ld)), M(Aff, bad_ld(s.p.add_ld)), M(Aff, bad_splits(s.p.a_splits)),
    M(Aff, bad_slab(s.p.a_slab)), M(Aff, s.cl = 0), M(Aff, bad_dtype(s.dtype))};
static const std::vector<TrainM> train_changes = {
    M(Train, bad_ptr(s.p.out)), M(Train, bad_ptr(s.p.a)), M(Train, bad_ptr(s.p.x)), M(Train, bad_ptr(s.p.mean)),
    M(Train, bad_ptr(s.p.rstd)), M(Train, bad_ptr(s.p.w)), M(Train, bad_ptr(s.p.part_x)), M(Train, bad_ptr(s.p.part_1)),
    M(Train, bad_ptr(s.p.vq)), M(Train, bad_ptr(s.p.vr)), M(Train, bad_ptr(s.p.add)), M(Train, bad_ptr(s.p.mask_src)),
    M(Train, s.p.nparts = pick({0, -1, 1})), M(Train, s.p.count = pick({0.0, -1.0, 1.0})), M(Train, bad_size(s.p.n)),
    M(Train, bad_size(s.p.c)), M(Train, bad_size(s.p.hw)), M(Train, bad_ld(s.p.out_ld)), M(Train, bad_ld(s.add_ld)),
    M(Train, bad_splits(s.p.a_splits)), M(Train, bad_slab(s.p.a_slab)), M(Train, bad_dtype(s.dtype))};
static const std::vector<AdjM> adj_changes = {
    M(Adj, bad_ptr(s.p.gx)), M(Adj, bad_ptr(s.p.gw)), M(Adj, bad_ptr(s.p.gb)), M(Adj, bad_ptr(s.p.gres)),
    M(Adj, bad_ptr(s.p.gy)), M(Adj, bad_ptr(s.p.gy2)), M(Adj, bad_ptr(s.p.x)), M(Adj, bad_ptr(s.p.mean)),
    M(Adj, bad_ptr(s.p.rstd)), M(Adj, bad_ptr(s.p.w)), M(Adj, bad_ptr(s.p.mask_src)), M(Adj, bad_splits(s.p.gy_splits)),
    M(Adj, bad_slab(s.p.gy_slab)), M(Adj, bad_splits(s.p.gy2_splits)), M(Adj, bad_slab(s.p.gy2_slab)),
    M(Adj, bad_size(s.p.n)), M(Adj, bad_size(s.p.c)), M(Adj, bad_size(s.p.hw)),
    M(Adj, s.p.row_blocks = pick({0, -1, 1, 2, 7, 1000})), M(Adj, s.cl = 0), M(Adj, bad_dtype(s.dtype))};

struct Lib {
#define F(name) decltype(&::name) name
  F(hf_chan_affine); F(hf_chan_affine_ex); F(hf_chan_affine_pair); F(hf_chan_affine_train); F(hf_chan_affine_train_pair);
  F(hf_chan_affine_bwd); F(hf_chan_affine_bwd_ex); F(hf_chan_affine_bwd_pair); F(hf_bn_adjoint_v4);
  F(hf_bn_adjoint_v4_pair);
#undef F
};

static Lib open_lib(const char* path) {
  void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!h) { std::printf("cannot load %s: %s\n", path, dlerror()); std::exit(2); }
  Lib l;
#define F(name) if (!(l.name = (decltype(&::name))dlsym(h, #name))) { std::printf("%s lacks " #name "\n", path); std::exit(2); }
  F(hf_chan_affine) F(hf_chan_affine_ex) F(hf_chan_affine_pair) F(hf_chan_affine_train) F(hf_chan_affine_train_pair)
  F(hf_chan_affine_bwd) F(hf_chan_affine_bwd_ex) F(hf_chan_affine_bwd_pair) F(hf_bn_adjoint_v4) F(hf_bn_adjoint_v4_pair)
#undef F
  return l;
}

static int aff_call(const Lib& l, int entry, const Aff* s) {
  const hf_affine_problem& p = s[0].p;
  if (entry == 0)
    return l.hf_chan_affine(p.out, p.a, p.x, p.mean, p.rstd, p.w, p.q, p.r, p.add, p.mask_src, p.relu_self, p.n, p.c,
                            p.hw, s[0].cl, p.out_ld, p.add_ld, s[0].dtype, nullptr);
  if (entry == 1)
    return l.hf_chan_affine_ex(p.out, p.a, p.x, p.mean, p.rstd, p.w, p.q, p.r, p.add, p.mask_src, p.relu_self, p.n, p.c,
                               p.hw, s[0].cl, p.out_ld, p.add_ld, p.a_splits, p.a_slab, s[0].dtype, nullptr);
  const hf_affine_problem two[2] = {s[0].p, s[1].p};
  return l.hf_chan_affine_pair(rnd(50) ? two : nullptr, s[0].dtype, nullptr);
}
static int train_call(const Lib& l, int entry, const Train* s) {
  const hf_affine_train_problem& p = s[0].p;
  if (entry == 0)
    return l.hf_chan_affine_train(p.out, p.a, p.x, p.mean, p.rstd, p.w, p.part_x, p.part_1, p.nparts, p.vq, p.vr,
                                  p.count, p.add, p.mask_src, p.n, p.c, p.hw, p.out_ld, s[0].add_ld, p.a_splits,
                                  p.a_slab, s[0].dtype, nullptr);
  hf_affine_train_problem two[2] = {s[0].p, s[1].p};
  if (rnd(4)) two[0].add = two[1].add = nullptr;  // (the paired form has no residual operand)
  return l.hf_chan_affine_train_pair(rnd(50) ? two : nullptr, s[0].dtype, nullptr);
}
static int adj_call(const Lib& l, int entry, const Adj* s) {
  const hf_bn_adjoint_problem& p = s[0].p;
  if (entry == 0)
    return l.hf_chan_affine_bwd(p.gx, p.gw, p.gb, p.gres, p.gy, p.gy2, p.x, p.mean, p.rstd, p.w, p.mask_src, p.n, p.c,
                                p.hw, s[0].cl, s[0].dtype, nullptr);
  if (entry == 1)
    return l.hf_chan_affine_bwd_ex(p.gx, p.gw, p.gb, p.gres, p.gy, p.gy_splits, p.gy_slab, p.gy2, p.gy2_splits,
                                   p.gy2_slab, p.x, p.mean, p.rstd, p.w, p.mask_src, p.n, p.c, p.hw, s[0].cl,
                                   p.row_blocks, s[0].dtype, nullptr);
  if (entry == 3)
    return l.hf_bn_adjoint_v4(p.gres, p.gx, p.gy, p.gy_splits, p.gy_slab, p.gy2, p.gy2_splits, p.gy2_slab, p.mask_src,
                              p.w, p.rstd, p.n * p.hw, p.c, s[0].dtype, nullptr);
  const hf_bn_adjoint_problem two[2] = {s[0].p, s[1].p};
  return entry == 2 ? l.hf_chan_affine_bwd_pair(rnd(50) ? two : nullptr, s[0].dtype, nullptr)
                    : l.hf_bn_adjoint_v4_pair(rnd(50) ? two : nullptr, s[0].dtype, nullptr);
}

struct Tally { long sets[3] = {0, 0, 0}, differ[3] = {0, 0, 0}, refused = 0, reached = 0; };

// `sets` argument sets for one entry point: two problems (the second one only read by the paired forms), 0 / 1 / 2
// changes spread over both; each library sees the same arguments (the generator is rewound for the second call).
template <typename S, typename Change, typename Call>
static Tally run(const char* name, long sets, bool paired, S (*base)(), const std::vector<Change>& changes, Call call,
                 const Lib& a, const Lib& b) {
  Tally t;
  for (long i = 0; i < sets; ++i) {
    S s[2] = {base(), base()};
    if (paired && s[0].p.c == 6) s[0].p.c = 8;
    const int k = pick({0, 1, 1, 1, 1, 1, 2, 2, 2, 2});
    for (int j = 0; j < k; ++j) changes[rnd((int)changes.size())](s[paired ? rnd(2) : 0]);
    const std::mt19937_64 at = rng;
    const int ra = call(a, s);
    rng = at;
    const int rb = call(b, s);
    ++t.sets[k];
    if (ra != rb) {
      if (++t.differ[k] <= 5) std::printf("  %s, %d change(s): %d vs %d\n", name, k, ra, rb);
    }
    (ra == HF_ERR_ARG || ra == HF_ERR_ALIGN ? t.refused : t.reached)++;
  }
  std::printf("%-28s sets %ld / %ld / %ld (0 / 1 / 2 changes), refused %ld, reached the launch %ld, differ %ld / %ld / %ld\n",
              name, t.sets[0], t.sets[1], t.sets[2], t.refused, t.reached, t.differ[0], t.differ[1], t.differ[2]);
  return t;
}

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: %s <old libhfpcg.so> <new libhfpcg.so> [sets per entry point]\n", argv[0]); return 2; }
  const Lib a = open_lib(argv[1]), b = open_lib(argv[2]);
  const long sets = argc > 3 ? std::atol(argv[3]) : 6000;
  typedef int (*Count)(int*);
  int devices = 0;
  Count count = (Count)dlsym(RTLD_DEFAULT, "hipGetDeviceCount");
  if (!count) {
    void* hip = dlopen("libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
    count = hip ? (Count)dlsym(hip, "hipGetDeviceCount") : nullptr;
  }
  if (!count || (count(&devices) == 0 && devices > 0)) {
    std::printf("a GPU is visible (or the runtime cannot be asked): the accepted sets carry fake pointers -- not run\n");
    return 2;
  }
  std::vector<Tally> all;
#define RUN(name, paired, base, changes, call, entry) \
  all.push_back(run(name, sets, paired, base, changes, [](const Lib& l, const auto* s) { return call(l, entry, s); }, a, b))
  RUN("hf_chan_affine", false, base_aff, aff_changes, aff_call, 0);
  RUN("hf_chan_affine_ex", false, base_aff, aff_changes, aff_call, 1);
  RUN("hf_chan_affine_pair", true, base_aff, aff_changes, aff_call, 2);
  RUN("hf_chan_affine_train", false, base_train, train_changes, train_call, 0);
  RUN("hf_chan_affine_train_pair", true, base_train, train_changes, train_call, 1);
  RUN("hf_chan_affine_bwd", false, base_adj, adj_changes, adj_call, 0);
  RUN("hf_chan_affine_bwd_ex", false, base_adj, adj_changes, adj_call, 1);
  RUN("hf_chan_affine_bwd_pair", true, base_adj, adj_changes, adj_call, 2);
  RUN("hf_bn_adjoint_v4", false, base_adj, adj_changes, adj_call, 3);
  RUN("hf_bn_adjoint_v4_pair", true, base_adj, adj_changes, adj_call, 4);
  long must = 0, other = 0, total = 0;
  for (const Tally& t : all) must += t.differ[0] + t.differ[1], other += t.differ[2], total += t.sets[0] + t.sets[1] + t.sets[2];
  std::printf("%ld sets in all; differing with at most one change: %ld (must be 0); with two changes: %ld\n", total, must,
              other);
  return must ? 1 : 0;
}
