// Run-time flag -> template argument: the one idiom of the inst_*.hip units for choosing a
// kernel instance.  Host code only.  A generic lambda receives the values as
// std::integral_constant objects (usable wherever a constant expression is wanted); what it does
// not name is not instantiated, so a combination that is not shipped is excluded with
// `if constexpr` in the lambda.
#pragma once

#include <type_traits>

namespace tc {
namespace host {

template <int N>
using int_c = std::integral_constant<int, N>;

// with_bools(f, b0, b1, ...) = f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...)
template <class F>
int with_bools(F&& f) {
  return f();
}
template <class F, class... Rest>
int with_bools(F&& f, bool b, Rest... rest) {
  auto bind = [&](auto c) {
    return with_bools([&](auto... cs) { return f(c, cs...); }, rest...);
  };
  return b ? bind(std::true_type{}) : bind(std::false_type{});
}

// with_int<N0, N1, ...>(n, f, miss) = f(int_c<Ni>{}) for n == Ni, miss() for any other n
template <int... Ns, class F, class Miss>
int with_int(int n, F&& f, Miss&& miss) {
  int status = 0;
  const bool hit = ((n == Ns && ((status = f(int_c<Ns>{})), true)) || ...);
  return hit ? status : miss();
}

}  // namespace host
}  // namespace tc
