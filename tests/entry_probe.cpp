// dss2::entry (csrc/dss2_entry.hpp) on its own: a host program with stand-in plan hooks and launch bodies that write what they
// receive into a log.  tests/test_entry_cpu.py compiles it with -fsanitize=address,undefined and runs it; a closure that kept a
// caller's pointer instead of a copy reads freed or overwritten memory on replay, which the sanitizer or the comparison reports.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "dss2_entry.hpp"

static bool g_recording = false;
static int g_recording_asked = 0;
static std::vector<std::function<int(void*)>> g_ops;
static char g_err[256] = "";

namespace dss2 {
bool plan_recording() { ++g_recording_asked; return g_recording; }
void plan_record(std::function<int(void*)> op) { g_ops.emplace_back(std::move(op)); }
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace dss2

struct Args { int a; double b; const float* dev; int tail[3]; };
struct Desc { long long len; int n; };

static std::string g_log;
static int g_failed = 0;

static void logf(const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_log += buf;
}
static std::string take_log() { std::string s; s.swap(g_log); return s; }

#define CHECK(cond) do { if (!(cond)) { ++g_failed; fprintf(stderr, "line %d: CHECK(%s) failed; log '%s', error '%s'\n", __LINE__, #cond, g_log.c_str(), g_err); } } while (0)

// a body like the library's: a leading constant, a required struct, an optional one, a table with its count, plain values, a struct by
// reference, the stream last
static int body_launch(const char* who, const Args* ap, const Args* opt, const Desc* descs, int n_desc, float x, const Desc& byref, void* stream) {
  logf("%s a=%d b=%g dev=%p tail=%d,%d,%d ", who, ap->a, ap->b, (const void*)ap->dev, ap->tail[0], ap->tail[1], ap->tail[2]);
  if (opt) logf("opt=%d ", opt->a); else logf("opt=null ");
  if (descs) for (int i = 0; i < n_desc; ++i) logf("d%d=%lld/%d ", i, descs[i].len, descs[i].n); else logf("descs=null ");
  logf("n=%d x=%g byref=%lld/%d stream=%p", n_desc, x, byref.len, byref.n, stream);
  return 7;      // (the body's return value must come back from entry() and from the replay)
}
static int plain_launch(void* stream) { logf("plain stream=%p", stream); return 0; }

static void* const S1 = reinterpret_cast<void*>(0x1000);
static void* const S2 = reinterpret_cast<void*>(0x2000);
static const float* const DEV = reinterpret_cast<const float*>(0xd000);

int main() {
  const Desc ref{99, 9};

  // 1. not recording: the body runs once, nothing is recorded, and plan_recording() was asked exactly once
  {
    Args a{1, 2.5, DEV, {3, 4, 5}}, o{11, 0, nullptr, {0, 0, 0}};
    Desc* d = new Desc[2]{{16, 3}, {20, 2}};
    g_recording_asked = 0;
    const int rc = dss2::entry(body_launch, S1, "eager", dss2::copied(&a, "probe"), dss2::copied(&o), dss2::kept(d, 2), 2, 0.5f, ref);
    CHECK(rc == 7 && g_ops.empty() && g_recording_asked == 1);
    CHECK(take_log() == "eager a=1 b=2.5 dev=0xd000 tail=3,4,5 opt=11 d0=16/3 d1=20/2 n=2 x=0.5 byref=99/9 stream=0x1000");
    delete[] d;
  }

  // 2. recording: the body runs once, one op is recorded; it replays with equal values after the caller's structs were overwritten
  //    and the caller's table was freed, and a second replay gives the same log
  g_recording = true;
  std::string eager;
  {
    Args* a = new Args{1, 2.5, DEV, {3, 4, 5}};
    Args o{11, 0, nullptr, {0, 0, 0}};
    Desc* d = new Desc[2]{{16, 3}, {20, 2}};
    Desc* r = new Desc{99, 9};
    const int rc = dss2::entry(body_launch, S1, "rec", dss2::copied(a, "probe"), dss2::copied(&o), dss2::kept(d, 2), 2, 0.5f, *r);
    CHECK(rc == 7 && g_ops.size() == 1);
    eager = take_log();
    CHECK(eager == "rec a=1 b=2.5 dev=0xd000 tail=3,4,5 opt=11 d0=16/3 d1=20/2 n=2 x=0.5 byref=99/9 stream=0x1000");
    memset(a, 0, sizeof(*a)); memset(&o, 0, sizeof(o)); memset(d, 0, 2 * sizeof(Desc)); memset(r, 0, sizeof(*r));
    delete a; delete[] d; delete r;
  }
  g_recording = false;
  const std::string expect = "rec a=1 b=2.5 dev=0xd000 tail=3,4,5 opt=11 d0=16/3 d1=20/2 n=2 x=0.5 byref=99/9 stream=0x2000";
  if (g_ops.size() == 1) {
    CHECK(g_ops[0](S2) == 7);
    CHECK(take_log() == expect);
    std::vector<std::function<int(void*)>> moved = std::move(g_ops);      // (a plan's vector may grow and move its ops)
    g_ops.clear();
    CHECK(moved[0](S2) == 7);
    CHECK(take_log() == expect);
  }
  g_ops.clear();

  // 3. a null optional struct replays as null; a table with a null pointer, or with a count <= 0, is null eagerly and on replay
  g_recording = true;
  {
    Args a{1, 2.5, DEV, {3, 4, 5}};
    Desc d[1] = {{16, 3}};
    dss2::entry(body_launch, S1, "nulls", dss2::copied(&a, "probe"), dss2::copied((const Args*)nullptr), dss2::kept((const Desc*)nullptr, 2), 2, 0.f, ref);
    dss2::entry(body_launch, S1, "zero", dss2::copied(&a, "probe"), dss2::copied((const Args*)nullptr), dss2::kept(d, 0), 0, 0.f, ref);
    dss2::entry(body_launch, S1, "minus", dss2::copied(&a, "probe"), dss2::copied((const Args*)nullptr), dss2::kept(d, -1), -1, 0.f, ref);
    CHECK(g_ops.size() == 3);
    const std::string e = take_log();
    CHECK(e.find("nulls a=1") != std::string::npos && e.find("opt=null descs=null n=2") != std::string::npos);
    CHECK(e.find("opt=null descs=null n=0") != std::string::npos && e.find("opt=null descs=null n=-1") != std::string::npos);
    CHECK(e.find("opt=1") == std::string::npos && e.find("d0=") == std::string::npos);
    g_recording = false;
    for (auto& op : g_ops) op(S1);
    CHECK(take_log() == e);      // (the same stream: the replay's log is the eager log, call for call)
  }
  g_ops.clear();

  // 4. the null-argument refusal: 2, the message, nothing recorded, nothing run -- recording or not
  for (int rec = 0; rec < 2; ++rec) {
    g_recording = rec != 0;
    g_err[0] = 0;
    const int rc = dss2::entry(body_launch, S1, "refused", dss2::copied((const Args*)nullptr, "dss2_probe"), dss2::copied((const Args*)nullptr), dss2::kept((const Desc*)nullptr, 0), 0, 0.f, ref);
    CHECK(rc == 2 && g_ops.empty() && g_log.empty());
    CHECK(std::string(g_err) == "dss2_probe: null argument");
  }

  // 5. a body with no argument but the stream
  g_recording = true;
  CHECK(dss2::entry(plain_launch, S1) == 0 && g_ops.size() == 1);
  g_recording = false;
  if (g_ops.size() == 1) CHECK(g_ops[0](S2) == 0);
  CHECK(take_log() == "plain stream=0x1000plain stream=0x2000");
  g_ops.clear();

  if (g_failed) { fprintf(stderr, "entry_probe: %d checks failed\n", g_failed); return 1; }
  printf("entry_probe: ok\n");
  return 0;
}
