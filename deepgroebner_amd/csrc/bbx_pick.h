// The one switch from a run-time shape number to a compile-time constant, for the launchers of the kernel files (bbx_launch.h).
// Plain C++17, nothing of HIP: tests/launch_pick_check.cpp runs it on the host.
#pragma once
#include <type_traits>

constexpr int BBX_PICK_NONE = 1;      // "no such instantiation" (bbx_launch.h: this is hipErrorInvalidValue)

// Calls f(std::integral_constant<int, V>{}) for the V among Vs that equals v and returns what f returned.  The template argument
// is the run-time value itself, so a cell cannot be routed to another cell's kernel; a value that is not listed is REFUSED:
// f is not called, nothing is launched, the result is `none`.  Where the cross product of nested picks holds cells for which no
// kernel exists, f cuts them with `if constexpr` and returns the same code.  (A left fold: the compiler then instantiates, and
// emits, the kernels a callback names in the order of the list.)
template <int... Vs, class F>
inline int bbx_pick(int v, F&& f, int none = BBX_PICK_NONE) {
  int rc = none;
  (void)(... || (v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)));
  return rc;
}
// ... and from a condition to std::true_type / std::false_type (a bool template argument takes no int)
template <class F>
inline int bbx_pick_bool(bool c, F&& f) { return c ? f(std::true_type{}) : f(std::false_type{}); }
