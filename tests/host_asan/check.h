// The sanitizer drivers' checks: a failed one prints where and ends the enclosing function
// (and with it the driver) with 1.  CHECK takes a condition, CHECK_OK an entry point's call
// (include/co_env.h before this header), which must return CO_OK.
#pragma once

#include <cstdio>

#define CHECK(x)                                                              \
  do {                                                                        \
    if (!(x)) {                                                               \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x);     \
      return 1;                                                               \
    }                                                                         \
  } while (0)

#define CHECK_OK(x)                                                           \
  do {                                                                        \
    int rc_ = (x);                                                            \
    if (rc_ != CO_OK) {                                                       \
      std::fprintf(stderr, "%s:%d: %s -> %d\n", __FILE__, __LINE__, #x, rc_); \
      return 1;                                                               \
    }                                                                         \
  } while (0)
