// Registry of measured launch plans (see tune.hpp).  Written before the first launch by the host binding and
// read-only afterwards; a mutex keeps concurrent registration / lookup well defined.
#include "common.hpp"
#include "tune.hpp"
#include <mutex>
#include <vector>

namespace {
struct Entry { int kind; int64_t a, b, c, d; TunePlan plan; int64_t hits, declines; };
std::vector<Entry>& table() { static std::vector<Entry> t; return t; }
std::mutex& mu() { static std::mutex m; return m; }
Entry* find(int kind, int64_t a, int64_t b, int64_t c, int64_t d) {
  for (Entry& e : table())
    if (e.kind == kind && e.a == a && e.b == b && e.c == c && e.d == d) return &e;
  return nullptr;
}
}  // namespace

bool creid_tune_lookup(int kind, int64_t a, int64_t b, int64_t c, int64_t d, TunePlan& out) {
  std::lock_guard<std::mutex> g(mu());
  Entry* e = find(kind, a, b, c, d);
  if (!e) return false;
  ++e->hits;
  out = e->plan;
  return true;
}

bool creid_tune_peek(int kind, int64_t a, int64_t b, int64_t c, int64_t d, TunePlan& out) {
  std::lock_guard<std::mutex> g(mu());
  const Entry* e = find(kind, a, b, c, d);
  if (e) out = e->plan;
  return e != nullptr;
}

void creid_tune_declined(int kind, int64_t a, int64_t b, int64_t c, int64_t d) {
  std::lock_guard<std::mutex> g(mu());
  if (Entry* e = find(kind, a, b, c, d)) ++e->declines;
}

extern "C" {

int creid_tune_set(int32_t kind, int64_t a, int64_t b, int64_t c, int64_t d, int32_t p0, int32_t p1, int32_t p2) {
  if (kind != CREID_TUNE_WGRAD && kind != CREID_TUNE_IGEMM) return CREID_E_ARG;
  std::lock_guard<std::mutex> g(mu());
  if (Entry* e = find(kind, a, b, c, d)) { e->plan = TunePlan{p0, p1, p2}; return 0; }
  table().push_back(Entry{kind, a, b, c, d, TunePlan{p0, p1, p2}, 0, 0});
  return 0;
}

int creid_tune_clear(void) {
  std::lock_guard<std::mutex> g(mu());
  table().clear();
  return 0;
}

int64_t creid_tune_count(int32_t kind, int64_t a, int64_t b, int64_t c, int64_t d, int32_t what) {
  if (what != 0 && what != 1) return -2;
  std::lock_guard<std::mutex> g(mu());
  const Entry* e = find(kind, a, b, c, d);
  if (!e) return -1;
  return what == 0 ? e->hits : e->declines;
}

}  // extern "C"
