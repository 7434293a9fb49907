// Signature codes of the C API: one letter per type, the return type first, then the parameters.
//   p  any pointer (hipStream_t included)    l  int64_t    i  int    u  uint64_t    f  float
// sig(&pa_xxx) is the code of a launcher as pa_api.h declares it; dispatch.cpp compares it at compile time with the
// code tools/build_native.py derives from the ctypes table (ops/_sigs.py), and picks the argument converter of the
// native entry points by the same letters. A type outside the set does not compile. No Python dependency.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string_view>
#include <type_traits>

namespace pa_sig {

template <typename T> struct unsupported : std::false_type {};

template <typename T> constexpr char code() {
  if constexpr (std::is_pointer_v<T>) return 'p';
  else if constexpr (std::is_same_v<T, int64_t>) return 'l';
  else if constexpr (std::is_same_v<T, int>) return 'i';
  else if constexpr (std::is_same_v<T, uint64_t>) return 'u';
  else if constexpr (std::is_same_v<T, float>) return 'f';
  else static_assert(unsupported<T>::value, "type T has no signature code: pointer, int64_t, int, uint64_t or float");
  return '?';
}

template <typename R, typename... A> struct Codes {
  static constexpr char value[] = {code<R>(), code<A>()..., '\0'};
};

template <typename R, typename... A> constexpr std::string_view sig(R (*)(A...)) {
  return std::string_view(Codes<R, A...>::value, 1 + sizeof...(A));
}

}  // namespace pa_sig
