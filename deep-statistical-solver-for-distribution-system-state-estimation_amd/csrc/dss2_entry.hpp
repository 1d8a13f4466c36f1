// The one spelling of a launch entry point: dss2::entry(launch_body, stream, arguments...).
//
// A launch plan (dss2_plan_*, dss2_api.hip) works because every launch entry point, while a plan records, appends a closure -- its own
// launch body bound to COPIES of its host-side arguments -- and then runs the same body eagerly; dss2_plan_run re-issues the closures
// in order from one C call.  entry() is that contract: an extern "C" entry is its checks (if any) and one call of entry().
//
// Plain arguments (numbers, device pointers, small structs passed by reference) are copied by value.  Two wrappers cover host memory
// that the caller may reuse or free after the call:
//   copied(p)         a struct behind a const T*: the closure owns a T and hands the body const T*; a null p stays null on replay.
//   copied(p, name)   the same for a struct the entry requires: a null p refuses the call with "<name>: null argument" (return 2),
//                     before anything is recorded or launched.
//   kept(p, n)        a host table of n elements: the closure owns a std::vector<T> and hands the body const T*.  A null p or n <= 0
//                     gives the body a null pointer, eagerly and on replay alike.
//
// Host-only: no HIP here, so a program with its own set_error, plan_recording and plan_record can test it (tests/entry_probe.cpp).
#pragma once
#include <functional>
#include <optional>
#include <tuple>
#include <type_traits>
#include <vector>

namespace dss2 {

void set_error(const char* fmt, ...);
bool plan_recording();
void plan_record(std::function<int(void*)> op);

template <class T> struct CopiedArg { const T* p; const char* required_by; };
template <class T> inline CopiedArg<T> copied(const T* p, const char* required_by = nullptr) { return {p, required_by}; }
template <class T> struct KeptArg { const T* p; long long n; };
template <class T> inline KeptArg<T> kept(const T* p, long long n) { return {p && n > 0 ? p : nullptr, n}; }

namespace entry_detail {

// what the eager call hands the launch body for an argument
template <class A> inline const A& now(const A& a) { return a; }
template <class T> inline const T* now(const CopiedArg<T>& a) { return a.p; }
template <class T> inline const T* now(const KeptArg<T>& a) { return a.p; }

template <class A> inline bool refused(const A&) { return false; }
template <class T> inline bool refused(const CopiedArg<T>& a) {
  if (a.p || !a.required_by) return false;
  set_error("%s: null argument", a.required_by);
  return true;
}

// what a recorded closure holds for an argument, and hands the launch body on replay
template <class A> struct Held {
  A v;
  explicit Held(const A& a) : v(a) {}
  const A& get() const { return v; }
};
template <class T> struct Held<CopiedArg<T>> {
  std::optional<T> v;
  explicit Held(const CopiedArg<T>& a) { if (a.p) v.emplace(*a.p); }
  const T* get() const { return v ? &*v : nullptr; }
};
template <class T> struct Held<KeptArg<T>> {
  std::vector<T> v;
  explicit Held(const KeptArg<T>& a) { if (a.p) v.assign(a.p, a.p + a.n); }
  const T* get() const { return v.empty() ? nullptr : v.data(); }
};

}  // namespace entry_detail

// Runs launch(args..., stream); while a plan records, first records the same call on copies of args.  Not recording, it costs
// plan_recording()'s one atomic load: the copies are built only under that branch.  (P...: the body's parameters, `void* stream` last.)
template <class... P, class... A>
inline int entry(int (*launch)(P...), void* stream, const A&... args) {
  using namespace entry_detail;
  if ((... || refused(args))) return 2;
  if (plan_recording())
    plan_record([launch, held = std::make_tuple(Held<std::decay_t<const A&>>(args)...)](void* s_) {
      return std::apply([&](const auto&... h) { return launch(h.get()..., s_); }, held);
    });
  return launch(now(args)..., stream);
}

}  // namespace dss2
