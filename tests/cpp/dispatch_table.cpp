// tests/cpp/dispatch_table.cpp — the value-to-tag matchers of nlsolver_amd/csrc/nlsg_dispatch.h on
// every named list: each listed value reaches its own tag once, every other value reaches nothing.
// Exit status 0 and "ok" when all hold; the first failure is printed and the status is 1.
#include <climits>
#include <cstdio>
#include <vector>

#include "../../nlsolver_amd/csrc/nlsg_dispatch.h"

using namespace nlsg;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
      failures++;                                                    \
    }                                                                \
  } while (0)

// `with(v, f)` is one of the named matchers. Listed values: the tag's value is v, f runs once, the
// answer is true. The first value below and above the list, the gaps, -1 and INT_MAX: f never runs,
// the answer is false.
template <typename With>
static void check_list(const char *name, With with, const std::vector<int> &listed, const std::vector<int> &gaps) {
  for (int v : listed) {
    int calls = 0, seen = INT_MIN;
    const bool matched = with(v, [&](auto tag) {
      calls++;
      seen = tag;  // (a tag converts to its value)
      static_assert(decltype(tag)::value == decltype(tag){}(), "a tag is an integral_constant");
    });
    if (!(matched && calls == 1 && seen == v)) {
      std::printf("%s: value %d -> matched %d, %d calls, tag %d\n", name, v, matched, calls, seen);
      failures++;
    }
  }
  std::vector<int> outside = gaps;
  outside.insert(outside.end(), {listed.front() - 1, listed.back() + 1, -1, INT_MAX});
  for (int v : outside) {
    bool is_listed = false;
    for (int l : listed) is_listed |= l == v;
    if (is_listed) continue;  // (-1 is BFGS-like lists' business, not of these)
    int calls = 0;
    const bool matched = with(v, [&](auto) { calls++; });
    if (matched || calls) {
      std::printf("%s: value %d outside the list -> matched %d, %d calls\n", name, v, matched, calls);
      failures++;
    }
  }
}

int main() {
  check_list("objective", [](int v, auto f) { return with_objective(v, f); },
             {NLSG_OBJ_ROSENBROCK, NLSG_OBJ_SPHERE, NLSG_OBJ_STYBLINSKI_TANG, NLSG_OBJ_RASTRIGIN}, {NLSG_OBJ_CUSTOM});
  check_list("chunks", [](int v, auto f) { return with_chunks(v, f); }, {1, 2, 4, 8}, {3, 5, 6, 7});
  check_list("groups", [](int v, auto f) { return with_groups(v, f); }, {4, 8, 16, 32}, {12, 5, 24, 64});
  check_list("batch groups", [](int v, auto f) { return with_batch_groups(v, f); }, {4, 8, 16, 32, 64}, {12, 48});
  check_list("a list spelled at its call site", [](int v, auto f) { return with_value<-1, 0, 1, 2, 3>(v, f); },
             {-1, 0, 1, 2, 3}, {});

  // with_bool: each value its own tag, once
  for (int b = 0; b < 2; b++) {
    int calls = 0, seen = -1;
    CHECK(with_bool(b != 0, [&](auto tag) {
      calls++;
      seen = tag ? 1 : 0;
    }));
    CHECK(calls == 1 && seen == b);
  }

  // a nest's answer is its innermost matcher's: one unmatched level anywhere makes the whole false
  int inner_calls = 0;
  CHECK(!with_objective(NLSG_OBJ_SPHERE, [&](auto) { return with_chunks(3, [&](auto) { inner_calls++; }); }));
  CHECK(!with_objective(7, [&](auto) { return with_chunks(2, [&](auto) { inner_calls++; }); }));
  CHECK(!with_bool(true, [&](auto) { return with_groups(12, [&](auto) { inner_calls++; }); }));
  CHECK(inner_calls == 0);
  CHECK(dispatch_call([&](auto a, auto b) { inner_calls += a + b; }, std::integral_constant<int, 2>{},
                      std::integral_constant<int, 3>{}));
  CHECK(inner_calls == 5);

  // objective x chunks x bool: the 32 inputs visit the 32 cells once each, each its own
  int visits[4][9][2] = {};
  const int chunk_values[4] = {1, 2, 4, 8};
  for (int obj = 0; obj < 4; obj++)
    for (int chunks : chunk_values)
      for (int vec = 0; vec < 2; vec++) {
        const bool matched = with_objective(obj, [&](auto O) {
          return with_chunks(chunks, [&](auto C) {
            return with_bool(vec != 0, [&](auto V) {
              constexpr int o = decltype(O)::value, c = decltype(C)::value;  // (compile-time, as a kernel's arguments)
              constexpr bool v = decltype(V)::value;
              static_assert(o >= 0 && o < 4 && c >= 1 && c <= 8, "tags carry the list's values");
              CHECK(o == obj && c == chunks && v == (vec != 0));
              visits[o][c][v]++;
            });
          });
        });
        CHECK(matched);
      }
  int cells = 0, total = 0;
  for (auto &per_obj : visits)
    for (auto &per_chunk : per_obj)
      for (int n : per_chunk) {
        CHECK(n == 0 || n == 1);
        cells += n == 1;
        total += n;
      }
  CHECK(cells == 32 && total == 32);

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
