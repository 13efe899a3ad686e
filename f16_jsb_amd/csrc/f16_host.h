// f16_host.h -- the host side's error handling, shared by every file that launches a kernel or
// answers an entry point: the thread's last error message (f16env_last_error), set_err, HIPCHK,
// and env_int for the F16ENV_* tuning variables. Needs the HIP runtime only; includes no project
// file.
#pragma once
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>

#include <string>

// ------------------------------------------------------------------------------------------
// error handling
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int set_err(int code, const char* msg) {
  g_err = msg;
  return code;
}
#define HIPCHK(x)                                                                   \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess) {                                                         \
      char b_[256];                                                                 \
      snprintf(b_, sizeof b_, "%s failed: %s", #x, hipGetErrorString(e_));          \
      return set_err(-2, b_);                                                       \
    }                                                                               \
  } while (0)

// An integer tuning variable of the environment (F16ENV_*), or `dflt` when it is not set. Read at
// create and by the cold launchers only: never on the path of a step.
static int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}
