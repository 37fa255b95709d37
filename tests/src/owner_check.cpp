// The rules of csrc/device_owner.h, checked on the CPU: Owned over malloc'd blocks with a counting release function. Built with
// AddressSanitizer + UBSan by tests/test_device_owner.py and run as an ordinary program; a block lost or released twice fails
// the run even where no CHECK looks. The HIP aliases are only instantiated empty: no device is touched.
#include "../../neuralampmodelercore_amd/csrc/device_owner.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace namhip;

static int g_released = 0;
static void* g_last = nullptr;
static hipError_t counting_free(void* p)
{
  g_released++;
  g_last = p;
  std::free(p);
  return hipSuccess;
}
static hipError_t refusing_free(void* p)
{
  std::free(p);
  return hipErrorInvalidValue;
}
using Buf = Owned<int, &counting_free>;

static int g_failures = 0;
#define CHECK(cond)                                                                                                    \
  do                                                                                                                   \
  {                                                                                                                    \
    if (!(cond))                                                                                                       \
    {                                                                                                                  \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);                                   \
      g_failures++;                                                                                                    \
    }                                                                                                                  \
  } while (0)

static int* fill(Buf& b)
{
  *b.out() = static_cast<int*>(std::malloc(64));
  return b.get();
}

struct Three // (the shape of WidthGroup / PersistSession: owners next to plain fields)
{
  Buf a, b, c;
  int plain = 7;
};

int main()
{
  { // the destructor releases once; an empty owner releases nothing
    Buf empty;
    Buf b;
    CHECK(!b && b.get() == nullptr);
    int* p = fill(b);
    CHECK(b && b.get() == p && g_released == 0);
  }
  CHECK(g_released == 1);

  { // move-construction: nothing released, the source empty, the block released once at the end
    g_released = 0;
    Buf a;
    int* p = fill(a);
    Buf b(std::move(a));
    CHECK(!a && a.get() == nullptr && b.get() == p && g_released == 0);
  }
  CHECK(g_released == 1);

  { // move-assignment releases what the target held, and only that
    g_released = 0;
    Buf a, b;
    int* pa = fill(a);
    int* pb = fill(b);
    b = std::move(a);
    CHECK(g_released == 1 && g_last == pb && b.get() == pa && !a);
    Buf& self = b; // self-move releases nothing and keeps the block
    b = std::move(self);
    CHECK(g_released == 1 && b.get() == pa);
    b = Buf(); // (how a struct of owners is cleared)
    CHECK(g_released == 2 && g_last == pa && !b);
  }
  CHECK(g_released == 2);

  { // reset(): the release function's answer; on an empty owner nothing is called
    g_released = 0;
    Buf a;
    CHECK(a.reset() == hipSuccess && g_released == 0);
    fill(a);
    CHECK(a.reset() == hipSuccess && g_released == 1 && !a);
    CHECK(a.reset() == hipSuccess && g_released == 1);
    Owned<int, &refusing_free> r;
    *r.out() = static_cast<int*>(std::malloc(16));
    CHECK(r.reset() == hipErrorInvalidValue && !r); // (refresh_map reports a refused hipFree)
    CHECK(r.reset() == hipSuccess);
  }

  { // out() on a non-empty owner does not lose the old block: it is released before the slot is handed out
    g_released = 0;
    Buf a;
    int* p1 = fill(a);
    int** slot = a.out();
    CHECK(g_released == 1 && g_last == p1 && *slot == nullptr && !a);
    *slot = static_cast<int*>(std::malloc(64));
    CHECK(a);
  }
  CHECK(g_released == 2);

  { // a vector of structs with three owners: resize up moves (releases nothing), resize down releases what it drops
    g_released = 0;
    std::vector<Three> v(2);
    for (Three& t : v)
      fill(t.a), fill(t.b), fill(t.c);
    int* first = v[0].a.get();
    v.resize(64); // (reallocates: every element is moved)
    CHECK(g_released == 0 && v[0].a.get() == first && v[1].c && !v[2].a && v[63].plain == 7);
    fill(v[63].b);
    v.resize(1);
    CHECK(g_released == 4); // element 1's three and element 63's one
    v[0] = Three(); // (free_group's successor)
    CHECK(g_released == 7 && !v[0].a && !v[0].b && !v[0].c);
    fill(v[0].c);
  }
  CHECK(g_released == 8);

  { // the HIP aliases, empty: destructors, reset() and moves call nothing
    DeviceBuf<float> d, d2(std::move(d));
    PinnedBuf<float> h;
    MappedBuf<unsigned> m, m2;
    StreamOwner s, s2;
    EventOwner e;
    s2 = std::move(s);
    m2 = std::move(m);
    CHECK(!d2 && !h && !m2 && m2.host() == nullptr && m2.dev() == nullptr && !s2 && !e);
    CHECK(d2.reset() == hipSuccess && h.reset() == hipSuccess && m2.reset() == hipSuccess && s2.reset() == hipSuccess
          && e.reset() == hipSuccess);
  }

  if (g_failures)
    return 1;
  std::puts("owner_check: ok");
  return 0;
}
