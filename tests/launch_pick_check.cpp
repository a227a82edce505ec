// Host check of bbx_pick / bbx_pick_bool (deepgroebner_amd/csrc/bbx_pick.h), the launchers' one switch from a run-time shape
// number to a template argument: every value list the library uses, unlisted values, nested picks, and an `if constexpr`
// refusal inside the callback.  A program of its own (tests/test_launch_pick_cpu.py builds it with the sanitizers).
#include <climits>
#include <cstdio>
#include <initializer_list>
#include <type_traits>

#include "bbx_pick.h"

static int failures = 0, checks = 0;
#define CHECK(...) do { checks++; if (!(__VA_ARGS__)) { failures++; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); } } while (0)

static const int UNLISTED[] = {0, -1, 5, 7, 33, INT_MAX};

// One list: each listed value calls f exactly once with that constant and bbx_pick returns what f returned (0 and non-zero);
// a value that is not listed calls nothing and returns the no-match code
template <int... Vs>
static void check_list() {
  const int listed[] = {Vs...};
  auto is_listed = [&](int v) { for (int w : listed) if (w == v) return true; return false; };
  for (int v : listed) {
    for (int ret : {0, 7001}) {
      int calls = 0, got = INT_MIN;
      const int rc = bbx_pick<Vs...>(v, [&](auto V) { static_assert(std::is_same<decltype(V), std::integral_constant<int, decltype(V)::value>>::value, "");
                                                      calls++; got = V(); return ret; });
      CHECK(calls == 1); CHECK(got == v); CHECK(rc == ret);
    }
  }
  for (int v : UNLISTED) {
    if (is_listed(v)) continue;                              // (0 is a member of {0, 1})
    int calls = 0;
    CHECK(bbx_pick<Vs...>(v, [&](auto) { calls++; return 0; }) == BBX_PICK_NONE);
    CHECK(calls == 0);
    CHECK(bbx_pick<Vs...>(v, [&](auto) { calls++; return 0; }, -77) == -77);   // (the no-match code as an argument)
    CHECK(calls == 0);
  }
}

// what a launcher's callback does with its constants: they are template arguments
template <int A, int B> static int cell() { return 1000 * A + B; }

int main() {
  check_list<2, 4, 8>();
  check_list<1, 2, 4, 8>();
  check_list<3, 6, 10, 16, 32>();
  check_list<3, 8, 16>();
  check_list<64, 128>();
  check_list<0, 1>();
  std::printf("lists cases %d failed %d\n", checks, failures);

  // two nested picks reach exactly the cell asked for: the full 4 x 5 table, and nothing for a value outside either list
  const int as[] = {1, 2, 4, 8}, bs[] = {3, 6, 10, 16, 32};
  int cells = 0;
  for (int a : as) for (int b : bs) {
    int calls = 0;
    const int rc = bbx_pick<1, 2, 4, 8>(a, [&](auto A) { return bbx_pick<3, 6, 10, 16, 32>(b, [&](auto B) { calls++; return cell<A(), B()>(); }); });
    CHECK(calls == 1); CHECK(rc == 1000 * a + b);
    cells++;
  }
  CHECK(cells == 20);
  for (int bad : UNLISTED) {
    int calls = 0;
    CHECK(bbx_pick<1, 2, 4, 8>(bad, [&](auto A) { return bbx_pick<3, 6, 10, 16, 32>(3, [&](auto B) { calls++; return cell<A(), B()>(); }); }) == BBX_PICK_NONE);
    CHECK(bbx_pick<1, 2, 4, 8>(4, [&](auto A) { return bbx_pick<3, 6, 10, 16, 32>(bad, [&](auto B) { calls++; return cell<A(), B()>(); }); }) == BBX_PICK_NONE);
    CHECK(calls == 0);
  }
  std::printf("nested cases %d failed %d\n", checks, failures);

  // an `if constexpr` refusal inside the callback returns its code and does not fall through to another cell (the binomial
  // policy kernels: 10 k-steps exist for W = 4 only, none at all for W = 8)
  for (int w : {2, 4, 8}) for (int ks : {6, 10}) {
    int launched = 0;
    const int rc = bbx_pick<2, 4, 8>(w, [&](auto W) { return bbx_pick<6, 10>(ks, [&](auto KS) {
      if constexpr (W() == 8 || (KS() == 10 && W() != 4)) return -5;
      else { launched++; return cell<W(), KS()>(); }
    }); });
    const bool exists = w != 8 && (ks == 6 || w == 4);
    CHECK(launched == (exists ? 1 : 0)); CHECK(rc == (exists ? 1000 * w + ks : -5));
  }
  // booleans
  for (bool c : {false, true}) {
    int calls = 0;
    CHECK(bbx_pick_bool(c, [&](auto C) { calls++; return std::integral_constant<bool, C()>::value ? 11 : 22; }) == (c ? 11 : 22));
    CHECK(calls == 1);
  }
  std::printf("refusal cases %d failed %d\n", checks, failures);
  return failures ? 1 : 0;
}
