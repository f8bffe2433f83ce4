// dispatch_test.cc -- stand-alone host test of l7m_dispatch.h
// (tests/test_dispatch_cpu.py builds it with g++ under ASan/UBSan): the value
// lists the launchers use -- hit modes {0, 1, 2}, end-code registers {4, 8, 0},
// slow-pass tiers {1, 2}, two bools (Kafka), kind & 3 (resident) -- reach the
// lambda as the constant equal to the runtime value, exactly once; nested
// dispatch visits every cell of the launchers' products exactly once; a value
// outside the list returns the fallback and calls nothing.
#include <cstdio>
#include <map>
#include <tuple>
#include <vector>

#include "../../cilium_amd/csrc/l7m_dispatch.h"

using l7m::dispatch_values;

static int g_fail = 0;
#define CHECK(c)                                           \
  do {                                                     \
    if (!(c)) {                                            \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                            \
    }                                                      \
  } while (0)

constexpr int kFallback = -77;

// One list: every listed value arrives as its own constant, once; values
// around the list arrive nowhere.
template <class T, T... Vs>
static void one_list(const std::vector<T>& unlisted) {
  for (const T v : {Vs...}) {
    int calls = 0;
    const int r = dispatch_values<T, Vs...>(v, kFallback, [&](auto K) {
      static_assert(std::is_same<typename decltype(K)::value_type, T>::value, "constant of the list's type");
      constexpr T k = decltype(K)::value;  // usable as a template argument
      ++calls;
      CHECK(k == v);
      return 1000 + static_cast<int>(k);
    });
    CHECK(calls == 1);
    CHECK(r == 1000 + static_cast<int>(v));
  }
  for (const T v : unlisted) {
    int calls = 0;
    const int r = dispatch_values<T, Vs...>(v, kFallback, [&](auto) {
      ++calls;
      return 0;
    });
    CHECK(calls == 0);
    CHECK(r == kFallback);
  }
}

template <int M, int R>
static int cell2() {
  return 10 * M + R;
}
template <int M, bool C, bool G>
static int cell3() {
  return 100 * M + 10 * C + G;
}

int main() {
  one_list<int, 0, 1, 2>({-1, 3, 4, 1 << 30});
  one_list<int, 4, 8, 0>({-1, 1, 2, 3, 5, 7, 9, 16});
  one_list<int, 1, 2>({0, 3, -1});
  one_list<bool, false, true>({});
  one_list<int, 0, 1, 2, 3>({-1, 4, 7});

  // hit mode x R: the first pass's 3 x 3 cells
  std::map<std::pair<int, int>, int> seen2;
  for (int mode = -1; mode <= 3; ++mode)
    for (int R : {-1, 0, 1, 4, 7, 8, 9}) {
      int calls = 0;
      const int r = dispatch_values<int, 0, 1, 2>(mode, kFallback, [&](auto M) {
        return dispatch_values<int, 4, 8, 0>(R, kFallback, [&](auto RR) {
          ++calls;
          ++seen2[{decltype(M)::value, decltype(RR)::value}];
          return cell2<decltype(M)::value, decltype(RR)::value>();
        });
      });
      const bool listed = mode >= 0 && mode <= 2 && (R == 4 || R == 8 || R == 0);
      CHECK(calls == (listed ? 1 : 0));
      CHECK(r == (listed ? 10 * mode + R : kFallback));
    }
  CHECK(seen2.size() == 9);
  for (const auto& kv : seen2) CHECK(kv.second == 1);

  // hit mode x client table in LDS x identity groups: Kafka's 3 x 2 x 2 cells
  std::map<std::tuple<int, bool, bool>, int> seen3;
  for (int mode = -1; mode <= 3; ++mode)
    for (bool cli : {false, true})
      for (bool groups : {false, true}) {
        int calls = 0;
        const int r = dispatch_values<int, 0, 1, 2>(mode, kFallback, [&](auto M) {
          return dispatch_values<bool, false, true>(cli, kFallback, [&](auto C) {
            return dispatch_values<bool, false, true>(groups, kFallback, [&](auto G) {
              ++calls;
              ++seen3[std::make_tuple(decltype(M)::value, decltype(C)::value, decltype(G)::value)];
              return cell3<decltype(M)::value, decltype(C)::value, decltype(G)::value>();
            });
          });
        });
        const bool listed = mode >= 0 && mode <= 2;
        CHECK(calls == (listed ? 1 : 0));
        CHECK(r == (listed ? 100 * mode + 10 * cli + groups : kFallback));
      }
  CHECK(seen3.size() == 12);
  for (const auto& kv : seen3) CHECK(kv.second == 1);

  // R x tier: the slow pass's 3 x 2 cells
  std::map<std::pair<int, int>, int> seen_slow;
  for (int R : {4, 8, 0})
    for (int tier : {1, 2}) {
      const int r = dispatch_values<int, 4, 8, 0>(R, kFallback, [&](auto RR) {
        return dispatch_values<int, 1, 2>(tier, kFallback, [&](auto T) {
          ++seen_slow[{decltype(RR)::value, decltype(T)::value}];
          return cell2<decltype(RR)::value, decltype(T)::value>();
        });
      });
      CHECK(r == 10 * R + tier);
    }
  CHECK(seen_slow.size() == 6);
  for (const auto& kv : seen_slow) CHECK(kv.second == 1);

  std::printf("failures=%d\n", g_fail);
  return g_fail ? 1 : 0;
}
