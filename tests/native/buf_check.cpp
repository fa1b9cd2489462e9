// buf_check.cpp — the growth logic of csrc/lins_buf.h on the CPU, under AddressSanitizer and UBSan
// (tests/test_buf_host.py): the part of the header that needs no ROCm, instantiated with a malloc-backed policy that
// counts its calls, logs their order, knows the blocks that are live and can be told to fail the k-th allocation.
//   buf_check grow | fail | move | group        one case each; exit 0 and "ok <case>" when every check holds
#define LINS_BUF_NO_HIP
#include "lins_buf.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <utility>

namespace {

struct CountMem {
  static int allocs, frees, fail_at;  // fail_at: the allocation (counted from 1, failed ones included) that fails; 0: none
  static size_t max_live, last_bytes;
  static std::string log;             // 'A' / 'F' per successful call, 'X' per failed allocation
  static std::set<void*> live;
  static int alloc(void** p, size_t bytes) {
    ++allocs;
    if (allocs == fail_at) {
      log += 'X';
      return 2;  // (hipErrorOutOfMemory's value; any non-zero int)
    }
    *p = std::malloc(bytes);
    std::memset(*p, 0xAB, bytes);  // (ASan: the block really has `bytes` bytes)
    live.insert(*p), last_bytes = bytes, log += 'A';
    if (live.size() > max_live) max_live = live.size();
    return 0;
  }
  static int free(void* p) {
    if (!live.erase(p)) {
      std::fprintf(stderr, "free of a block that is not live\n");
      std::exit(1);
    }
    ++frees, log += 'F';
    std::free(p);
    return 0;
  }
  static void restart() { allocs = frees = fail_at = 0, max_live = last_bytes = 0, log.clear(); }
};
int CountMem::allocs = 0, CountMem::frees = 0, CountMem::fail_at = 0;
size_t CountMem::max_live = 0, CountMem::last_bytes = 0;
std::string CountMem::log;
std::set<void*> CountMem::live;

template <class T>
using B = lins::Buf<T, CountMem>;
using M = CountMem;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s  [log %s]\n", __FILE__, __LINE__, #c, M::log.c_str()); \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

void case_grow() {
  {
    B<double> b;
    CHECK(b.get() == nullptr && b.cap() == 0);
    CHECK(b.grow(0) == 0 && b.cap() == 1 && b.get() && M::allocs == 1 && M::last_bytes == sizeof(double));
    double* p0 = b;
    CHECK(b.grow(1) == 0 && b.grow(0) == 0 && b.get() == p0 && M::log == "A");  // within capacity: no policy call
    CHECK(b.grow(100) == 0 && b.cap() == 100 && M::last_bytes == 100 * sizeof(double));
    CHECK(M::log == "AFA" && M::max_live == 1);  // one free, then one allocation; never two live blocks
    b[99] = 1.0;
    double* p1 = b;
    CHECK(b.grow(100) == 0 && b.grow(7) == 0 && b.get() == p1 && b.cap() == 100 && M::log == "AFA");  // grow-only
    b.reset();
    CHECK(b.get() == nullptr && b.cap() == 0 && M::log == "AFAF");
    b.reset();  // (empty: nothing to free)
    CHECK(M::log == "AFAF");
    CHECK(b.grow(3) == 0 && b.cap() == 3);
  }
  CHECK(M::log == "AFAFAF" && M::live.empty() && M::allocs == M::frees);
}

void case_fail() {
  {
    B<int> b;
    CHECK(b.grow(10) == 0);
    M::fail_at = 2;
    CHECK(b.grow(20) == 2);  // the policy's error comes back
    CHECK(b.get() == nullptr && b.cap() == 0 && M::log == "AFX" && M::live.empty());  // old block freed first, buffer empty
    CHECK(b.grow(5) == 0 && b.cap() == 5 && b.get() && M::log == "AFXA");  // the next growth succeeds
    B<int> never;
    M::fail_at = M::allocs + 1;
    CHECK(never.grow(1) == 2 && never.get() == nullptr && never.cap() == 0);
  }
  CHECK(M::live.empty() && M::frees == 2 && M::allocs == 4);  // (2 of the 4 allocations failed) nothing leaks, nothing freed twice
}

struct Three {  // the PgMem pattern: *m = Three() releases what the members hold
  B<double> a, b;
  B<int> c;
  int n = 0;
};

void case_move() {
  {
    B<float> a;
    CHECK(a.grow(8) == 0);
    float* pa = a;
    B<float> b(std::move(a));  // move construction: the source is empty, nothing is allocated or freed
    CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == pa && b.cap() == 8 && M::log == "A");
    B<float> c;
    CHECK(c.grow(4) == 0);
    c = std::move(b);  // move assignment: the destination's old block is freed once
    CHECK(b.get() == nullptr && b.cap() == 0 && c.get() == pa && c.cap() == 8 && M::log == "AAF" && M::live.size() == 1);
    B<float>& self = c;
    c = std::move(self);
    CHECK(c.get() == pa && c.cap() == 8 && M::log == "AAF");
  }
  CHECK(M::log == "AAFF" && M::live.empty());
  M::restart();
  {
    Three t;
    CHECK(t.a.grow(3) == 0 && t.b.grow(4) == 0 && t.c.grow(5) == 0);
    t.n = 7;
    t = Three();
    CHECK(M::frees == 3 && M::live.empty() && !t.a.get() && !t.b.get() && !t.c.get() && t.a.cap() + t.b.cap() + t.c.cap() == 0 && t.n == 0);
    CHECK(t.b.grow(2) == 0);
  }
  CHECK(M::allocs == 4 && M::frees == 4 && M::live.empty());
}

void case_group() {
  {
    B<float> a;
    B<unsigned> b;
    B<char> c;
    CHECK(lins::grow_all(a, 10, b, 20, c, 5) == 0);  // all grow when the first is short
    CHECK(a.cap() == 10 && b.cap() == 20 && c.cap() == 5 && M::log == "AAA");
    float* pa = a;
    unsigned* pb = b;
    char* pc = c;
    CHECK(lins::grow_all(a, 10, b, 2000, c, 5000) == 0 && lins::grow_all(a, 0, b, 0, c, 0) == 0);  // the first answers for the group
    CHECK(a.get() == pa && b.get() == pb && c.get() == pc && M::log == "AAA");
    CHECK(lins::grow_all(a, 11, b, 22, c, 6) == 0);
    CHECK(M::log == "AAAFFFAAA" && a.cap() == 11 && b.cap() == 22 && c.cap() == 6);  // all freed first, then allocated in the order written
    M::fail_at = M::allocs + 2;  // the second allocation of the next growth
    CHECK(lins::grow_all(a, 12, b, 24, c, 7) == 2);
    CHECK(M::log == "AAAFFFAAAFFFAXF" && M::live.empty());  // every block obtained was returned
    CHECK(!a.get() && !b.get() && !c.get() && a.cap() == 0 && b.cap() == 0 && c.cap() == 0);
    CHECK(lins::grow_all(a, 1, b, 1, c, 1) == 0 && M::live.size() == 3);
    B<int> single;
    CHECK(lins::grow_all(single, 0) == 0 && single.cap() == 1);  // one member, and the clamp
  }
  CHECK(M::live.empty() && M::allocs - 1 == M::frees);  // (one allocation failed)
}

}  // namespace

int main(int argc, char** argv) {
  const std::string which = argc > 1 ? argv[1] : "";
  M::restart();
  if (which == "grow") case_grow();
  else if (which == "fail") case_fail();
  else if (which == "move") case_move();
  else if (which == "group") case_group();
  else return 2;
  std::printf("ok %s\n", which.c_str());
  return 0;
}
