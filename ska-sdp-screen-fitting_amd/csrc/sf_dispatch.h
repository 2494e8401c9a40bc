// sf_dispatch.h -- run-time value -> template-argument dispatch of the host
// launchers.  No kernel lives here: a unit that includes it gains no symbol.
#pragma once
#include <type_traits>

namespace sf {

// f(std::bool_constant<b>{}...) for run-time bools b...: the callable reads
// them as template arguments (decltype(B)::value).  Every combination of the
// bools instantiates f's body, so f guards the kernel variants that do not
// exist with `if constexpr` -- a kernel named in a discarded branch is never
// instantiated.
template <bool... Bs, class F>
void with_bools(F&& f) {
  f(std::bool_constant<Bs>{}...);
}
template <bool... Bs, class F, class... Rest>
void with_bools(F&& f, bool b, Rest... rest) {
  if (b)
    with_bools<Bs..., true>(f, rest...);
  else
    with_bools<Bs..., false>(f, rest...);
}

// The integer analogue: f(std::integral_constant<int, R>{}) for a run-time
// 1 <= R <= MAXR, the constant 0 for every other R; f maps each of 0..MAXR
// to a kernel that exists.
template <int MAXR, class F>
void with_radius(int R, F&& f) {
  if constexpr (MAXR >= 1) {
    if (R != MAXR) return with_radius<MAXR - 1>(R, f);
  }
  f(std::integral_constant<int, (MAXR >= 1 ? MAXR : 0)>{});
}

}  // namespace sf
