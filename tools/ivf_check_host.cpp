// Stand-alone host program over csrc/ivf_check.h, the checks rr_bank_load_ivf makes of a caller's inverted file before it allocates:
// good and bad files on exactly sized heap arrays, so that a sanitizer sees any read outside offsets [C + 1] or pids [offsets[C]].
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ivf_check_host.cpp -o tools/bin/ivf_check_host
//   tools/bin/ivf_check_host        (prints one line per case; exit status 0 when every case gave the expected verdict)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../reranking-multimodal-retrievers_amd/csrc/ivf_check.h"

static int failures = 0;

static void expect(const char* name, const std::vector<int64_t>& off, const std::vector<int32_t>& pid, int64_t passages, bool want_ok,
                   int want_list, int64_t want_longest, const char* want_word) {
  // exact-size heap copies: the vectors' capacity could hide an overrun
  int64_t* o = new int64_t[off.size()];
  int32_t* p = new int32_t[pid.size() ? pid.size() : 1];
  memcpy(o, off.data(), off.size() * sizeof(int64_t));
  if (!pid.empty()) memcpy(p, pid.data(), pid.size() * sizeof(int32_t));
  int64_t longest = -1;
  int list = -1;
  char why[160] = "";
  const bool ok = rr_ivf_check_host(o, pid.empty() ? nullptr : p, (int)off.size() - 1, passages, &longest, &list, why, sizeof why);
  const bool pass = ok == want_ok && (ok ? longest == want_longest : (list == want_list && strstr(why, want_word) != nullptr));
  printf("%-28s %s  ok=%d list=%d longest=%lld  %s\n", name, pass ? "PASS" : "FAIL", (int)ok, list, (long long)longest, why);
  if (!pass) ++failures;
  delete[] o;
  delete[] p;
}

int main() {
  const std::vector<int64_t> off{0, 3, 3, 5, 9};
  const std::vector<int32_t> pid{0, 4, 9, 2, 3, 0, 1, 8, 9};
  expect("good", off, pid, 10, true, 0, 4, "");
  expect("empty lists only", {0, 0, 0}, {}, 10, true, 0, 0, "");
  expect("one list of every passage", {0, 3}, {0, 1, 2}, 3, true, 0, 3, "");
  expect("offsets[0] = 1", {1, 3, 3, 5, 9}, pid, 10, false, 0, 0, "offsets[0]");
  expect("a decreasing offset", {0, 3, 2, 5, 9}, pid, 10, false, 1, 0, "decrease");
  expect("a huge offset then less", {0, (int64_t)1 << 40, 9}, pid, 10, false, 1, 0, "decrease");
  expect("a negative total", {0, -4}, {}, 10, false, 0, 0, "decrease");
  expect("pid = passages", off, {0, 4, 9, 2, 3, 0, 1, 8, 10}, 10, false, 3, 0, "names passage 10");
  expect("pid = -1", off, {0, 4, 9, -1, 3, 0, 1, 8, 9}, 10, false, 2, 0, "names passage -1");
  expect("a descending pair", off, {0, 9, 4, 2, 3, 0, 1, 8, 9}, 10, false, 0, 0, "ascend");
  expect("a duplicate", off, {0, 4, 9, 2, 3, 0, 1, 1, 9}, 10, false, 3, 0, "ascend");
  expect("a list longer than the bank", {0, 4}, {0, 1, 2, 2}, 3, false, 0, 0, "holds 4 entries");
  printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
