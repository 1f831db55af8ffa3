// Host-side helpers shared by the engines' host code. Nothing here includes
// a HIP header: now_s() serves the host-only dist server too, and HIP_CHECK
// names HIP symbols only where it is expanded.
#pragma once
#include <chrono>
#include <stdexcept>
#include <string>

inline double now_s() {
  using clk = std::chrono::steady_clock;
  return std::chrono::duration<double>(clk::now().time_since_epoch()).count();
}

// Throws "<HIP_CHECK_WHO>: <hip error> @ <expression>". The including file
// defines HIP_CHECK_WHO (its engine's name) before the first use.
#define HIP_CHECK(x)                                                       \
  do {                                                                     \
    hipError_t _e = (x);                                                   \
    if (_e != hipSuccess)                                                  \
      throw std::runtime_error(std::string(HIP_CHECK_WHO ": ") +           \
                               hipGetErrorString(_e) + " @ " #x);          \
  } while (0)
