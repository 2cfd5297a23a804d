// nlsolver_amd/csrc/nlsg_dispatch.h — run-time value to compile-time tag, for the launch sites of
// the engine files: which kernel instantiation runs is picked from the objective, the row width
// class, the lane-group size and the row alignment. Host only, plain C++17: no kernel header
// includes it and the run-time compiler never sees it.
//
//   routed(with_objective(obj, [&](auto O) {
//     return with_chunks(chunks, [&](auto C) {
//       return with_bool(vec, [&](auto V) { hipLaunchKernelGGL((kernel<O, C, V>), ...); });
//     });
//   }));
//
// A tag is a std::integral_constant, so it converts to its value in a template argument list, and
// nested generic lambdas instantiate exactly the cross product they name. A value outside its list
// matches nothing: no call is made and the result is false, never "the last case" (the launch site
// reports it, `routed` in nlsg_engine.h).
#pragma once
#include <type_traits>
#include <utility>

#include "nlsg_c_api.h"

namespace nlsg {

// f(tags...): a callback that returns void counts as matched, one that returns bool (a nested
// with_*) passes its own answer on
template <typename F, typename... Tags>
bool dispatch_call(F &&f, Tags... tags) {
  if constexpr (std::is_void_v<decltype(f(tags...))>) {
    f(tags...);
    return true;
  } else {
    return f(tags...);
  }
}

// calls f(std::integral_constant<int, Vk>{}) for the one Vk == v; false when no Vk matches or f says so
template <int... Vs, typename F>
bool with_value(int v, F &&f) {
  return ((v == Vs && dispatch_call(f, std::integral_constant<int, Vs>{})) || ...);
}

template <typename F>
bool with_bool(bool b, F &&f) {
  return b ? dispatch_call(f, std::true_type{}) : dispatch_call(f, std::false_type{});
}

// the lists that recur: the built-in objectives, 128-coordinate chunks of a row held in registers,
// lanes per row where several rows share a wave (up to a whole wave in the resident batch engines)
template <typename F>
bool with_objective(int obj, F &&f) {
  return with_value<NLSG_OBJ_ROSENBROCK, NLSG_OBJ_SPHERE, NLSG_OBJ_STYBLINSKI_TANG, NLSG_OBJ_RASTRIGIN>(
      obj, std::forward<F>(f));
}
template <typename F>
bool with_chunks(int chunks, F &&f) {
  return with_value<1, 2, 4, 8>(chunks, std::forward<F>(f));
}
template <typename F>
bool with_groups(int group, F &&f) {
  return with_value<4, 8, 16, 32>(group, std::forward<F>(f));
}
template <typename F>
bool with_batch_groups(int group, F &&f) {
  return with_value<4, 8, 16, 32, 64>(group, std::forward<F>(f));
}
// lanes per row of D coordinates, two to a lane. Past 64 coordinates a row takes the whole wave: 64 where
// that is one more group size (the resident batch engines), 0 where other kernels take over
inline int lane_group_of(uint64_t D, bool whole_wave) {
  return D <= 8 ? 4 : D <= 16 ? 8 : D <= 32 ? 16 : D <= 64 ? 32 : whole_wave ? 64 : 0;
}

}  // namespace nlsg
