// What rr_bank_load_ivf (include/rerank_mi355.h) checks of a caller's inverted file before anything is allocated, in plain host
// C++ (no HIP: a stand-alone program can include it): offsets [C + 1] start at 0 and do not decrease, every entry of pids
// [offsets[C]] lies in [0, passages) and every list ascends strictly.  The offsets are judged in full before a pid is read, so
// nothing outside pids [0, offsets[C]) is touched.
#pragma once
#include <stdint.h>
#include <stdio.h>

// true: fine, *longest_out = the longest list.  false: *list_out = the first offending list and `why` (why_len > 0) says what is
// wrong with it.
inline bool rr_ivf_check_host(const int64_t* offsets, const int32_t* pids, int C, int64_t passages, int64_t* longest_out, int* list_out,
                              char* why, size_t why_len) {
  *longest_out = 0;
  *list_out = 0;
  if (offsets[0] != 0) {
    snprintf(why, why_len, "offsets[0] = %lld, not 0", (long long)offsets[0]);
    return false;
  }
  for (int c = 0; c < C; ++c)
    if (offsets[c + 1] < offsets[c]) {
      *list_out = c;
      snprintf(why, why_len, "offsets decrease at list %d (%lld, then %lld)", c, (long long)offsets[c], (long long)offsets[c + 1]);
      return false;
    }
  int64_t longest = 0;
  for (int c = 0; c < C; ++c) {
    const int64_t n = offsets[c + 1] - offsets[c];
    if (n > passages) {
      *list_out = c;
      snprintf(why, why_len, "list %d holds %lld entries, the bank %lld passages", c, (long long)n, (long long)passages);
      return false;
    }
    for (int64_t i = offsets[c]; i < offsets[c + 1]; ++i) {
      const int32_t p = pids[i];
      if (p < 0 || p >= passages) {
        *list_out = c;
        snprintf(why, why_len, "list %d names passage %d, the bank holds %lld", c, p, (long long)passages);
        return false;
      }
      if (i > offsets[c] && p <= pids[i - 1]) {
        *list_out = c;
        snprintf(why, why_len, "list %d does not ascend strictly (%d behind %d)", c, p, pids[i - 1]);
        return false;
      }
    }
    if (n > longest) longest = n;
  }
  *longest_out = longest;
  return true;
}
