// tools/fh_memory_check.cpp -- the four owning types of fredholm_amd/csrc/fh_memory.h as a stand-alone program, for the tests and the host sanitizers.
// From the repository root:
//   g++ -std=c++17 -O1 -Wall -Werror tools/fh_memory_check.cpp -o fh_memory_check && ./fh_memory_check
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/fh_memory_check.cpp -o fh_memory_check && ./fh_memory_check
// Needs no GPU and no library: FH_MEMORY_FAKE_SEAM makes the header leave the HIP names and the eight raw_ functions of its seam to this file, which counts every
// call, backs buffers with malloc (so the sanitizers see a double free or a leak of the types themselves) and fails the allocation or creation it is told to.
// Prints "fh_memory_check: ok" or the number of failures.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
struct FakeEvent { int id; };
struct FakeStream { int id; unsigned flags; int priority; };
typedef FakeEvent* hipEvent_t;
typedef FakeStream* hipStream_t;

#define FH_MEMORY_FAKE_SEAM
#include "../fredholm_amd/csrc/fh_memory.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// the fake: live blocks with their sizes per kind (0 device, 1 pinned), counts of calls, and the number of acquisitions from now on that still succeed (-1: all)
static std::map<void*, size_t> g_blocks[2];
static int g_allocs[2], g_frees[2], g_bad_frees, g_events_made, g_events_gone, g_streams_made, g_streams_gone, g_fail_after = -1;
static size_t g_last_bytes;
static bool refused()
{
  if (g_fail_after < 0) return false;
  if (g_fail_after == 0) { g_fail_after = -1; return true; }
  --g_fail_after;
  return false;
}
static hipError_t fake_malloc(int kind, void** p, size_t bytes)
{
  if (refused()) return hipErrorOutOfMemory;
  *p = std::malloc(bytes);
  g_blocks[kind][*p] = bytes; g_last_bytes = bytes; ++g_allocs[kind];
  return hipSuccess;
}
static hipError_t fake_free(int kind, void* p)
{
  if (!g_blocks[kind].erase(p)) { ++g_bad_frees; return hipErrorOutOfMemory; }  // not live, or of the other kind: counted, not freed again
  std::free(p); ++g_frees[kind];
  return hipSuccess;
}
namespace fh { namespace seam {
hipError_t raw_device_malloc(void** p, size_t bytes) { return fake_malloc(0, p, bytes); }
hipError_t raw_device_free(void* p) { return fake_free(0, p); }
hipError_t raw_host_malloc(void** p, size_t bytes) { return fake_malloc(1, p, bytes); }
hipError_t raw_host_free(void* p) { return fake_free(1, p); }
hipError_t raw_event_create(hipEvent_t* e, unsigned) { if (refused()) return hipErrorOutOfMemory; *e = new FakeEvent{++g_events_made}; return hipSuccess; }
hipError_t raw_event_destroy(hipEvent_t e) { delete e; ++g_events_gone; return hipSuccess; }
hipError_t raw_stream_create(hipStream_t* s, unsigned flags, int priority) { if (refused()) return hipErrorOutOfMemory; *s = new FakeStream{++g_streams_made, flags, priority}; return hipSuccess; }
hipError_t raw_stream_destroy(hipStream_t s) { delete s; ++g_streams_gone; return hipSuccess; }
} }

static uint64_t live_count() { return fh::seam::live_count.load(); }
static uint64_t live_bytes() { return fh::seam::live_bytes.load(); }

template <typename B>
static void check_buffer(int kind)
{
  int& allocs = g_allocs[kind]; int& frees = g_frees[kind];
  const int a0 = allocs, f0 = frees;
  const uint64_t c0 = live_count(), b0 = live_bytes();
  {
    B b;
    EXPECT(b.get() == nullptr && b.size() == 0 && !b);
    EXPECT(b.ensure(0) == hipSuccess && b.get() == nullptr && allocs == a0);  // (nothing asked for, nothing made)
    // alloc(0): a real allocation of 16 bytes
    EXPECT(b.alloc(0) == hipSuccess && b.get() != nullptr && b.size() == 0 && g_last_bytes == 16 && allocs == a0 + 1);
    EXPECT(live_count() == c0 + 1 && live_bytes() == b0 + 16);
    // alloc over a live buffer frees it exactly once; three 4-byte elements are padded to 16, five are 20
    EXPECT(b.alloc(3) == hipSuccess && b.size() == 3 && g_last_bytes == 16 && allocs == a0 + 2 && frees == f0 + 1);
    EXPECT(b.alloc(5) == hipSuccess && b.size() == 5 && g_last_bytes == 20 && allocs == a0 + 3 && frees == f0 + 2);
    EXPECT(live_count() == c0 + 1 && live_bytes() == b0 + 20);
    // ensure: large enough is left alone (same block, no call), smaller never shrinks, larger reallocates
    auto* const p5 = b.get();
    EXPECT(b.ensure(5) == hipSuccess && b.ensure(2) == hipSuccess && b.ensure(0) == hipSuccess && b.get() == p5 && b.size() == 5 && allocs == a0 + 3 && frees == f0 + 2);
    EXPECT(b.ensure(6) == hipSuccess && b.size() == 6 && allocs == a0 + 4 && frees == f0 + 3 && live_bytes() == b0 + 24);
    // a failed alloc / ensure: empty, the old block freed exactly once, nothing counted as live
    g_fail_after = 0;
    EXPECT(b.alloc(7) == hipErrorOutOfMemory && b.get() == nullptr && b.size() == 0 && allocs == a0 + 4 && frees == f0 + 4);
    EXPECT(live_count() == c0 && live_bytes() == b0);
    EXPECT(b.alloc(4) == hipSuccess && frees == f0 + 4);  // (nothing to free after the failure)
    g_fail_after = 0;
    EXPECT(b.ensure(9) == hipErrorOutOfMemory && b.get() == nullptr && b.size() == 0 && frees == f0 + 5 && live_count() == c0);
    b.reset(); b.reset();
    EXPECT(frees == f0 + 5);
    // move construction and move assignment hand the block over; what the target held is freed
    B x, y;
    EXPECT(x.alloc(8) == hipSuccess && y.alloc(2) == hipSuccess);
    auto* const px = x.get();
    B z(std::move(x));
    EXPECT(z.get() == px && z.size() == 8 && x.get() == nullptr && x.size() == 0 && frees == f0 + 5);
    y = std::move(z);
    EXPECT(y.get() == px && y.size() == 8 && z.get() == nullptr && frees == f0 + 6 && live_count() == c0 + 1 && live_bytes() == b0 + 32);
    B& self = y;
    y = std::move(self);  // (self-assignment keeps the block)
    EXPECT(y.get() == px && frees == f0 + 6);
    // release: the caller's from now on, not freed and no longer counted
    auto* const raw = y.release();
    EXPECT(raw == px && y.get() == nullptr && y.size() == 0 && frees == f0 + 6 && live_count() == c0 && live_bytes() == b0);
    EXPECT(fake_free(kind, raw) == hipSuccess);
    --frees;  // (this program's own free, not the type's)
    // the destructor frees exactly once
    { B d; EXPECT(d.alloc(10) == hipSuccess); }
    EXPECT(frees == f0 + 7);
    { B d; }
    EXPECT(frees == f0 + 7);
  }
  EXPECT(frees == f0 + 7 && allocs - a0 == frees - f0 + 1);  // (+ 1: the released block)
  EXPECT(live_count() == c0 && live_bytes() == b0 && g_blocks[kind].empty() && g_bad_frees == 0);
}

static void check_vector()
{
  const int f0 = g_frees[0];
  {
    std::vector<fh::DeviceBuffer<uint8_t>> v;
    std::vector<uint8_t*> seen;
    for (int k = 0; k < 100; ++k) {  // (grows through several reallocations of the vector)
      fh::DeviceBuffer<uint8_t> b;
      EXPECT(b.alloc(100 + k) == hipSuccess);
      seen.push_back(b.get());
      v.push_back(std::move(b));
    }
    EXPECT(g_frees[0] == f0 && live_count() == 100);
    for (int k = 0; k < 100; ++k) EXPECT(v[k].get() == seen[k] && v[k].size() == (size_t)(100 + k));
    v.erase(v.begin());
    EXPECT(g_frees[0] == f0 + 1 && v[0].get() == seen[1]);
  }
  EXPECT(g_frees[0] == f0 + 100 && g_bad_frees == 0 && live_count() == 0 && live_bytes() == 0);
}

static void check_handles()
{
  {
    fh::Event e;
    EXPECT((hipEvent_t)e == nullptr);
    EXPECT(e.create() == hipSuccess && (hipEvent_t)e != nullptr && g_events_made == 1 && live_count() == 1 && live_bytes() == 0);
    EXPECT(e.create(2u) == hipSuccess && g_events_made == 2 && g_events_gone == 1 && live_count() == 1);  // (over a live one: destroyed once)
    g_fail_after = 0;
    EXPECT(e.create() == hipErrorOutOfMemory && (hipEvent_t)e == nullptr && g_events_gone == 2 && live_count() == 0);
    fh::Event a, b;
    EXPECT(a.create() == hipSuccess && b.create() == hipSuccess);
    const hipEvent_t ha = a;
    fh::Event c(std::move(a));
    EXPECT((hipEvent_t)c == ha && (hipEvent_t)a == nullptr && g_events_gone == 2);
    b = std::move(c);
    EXPECT((hipEvent_t)b == ha && (hipEvent_t)c == nullptr && g_events_gone == 3 && live_count() == 1);
    std::vector<fh::Event> pool;
    for (int k = 0; k < 40; ++k) { fh::Event n; EXPECT(n.create() == hipSuccess); pool.push_back(std::move(n)); }
    fh::Event back = std::move(pool.back());
    pool.pop_back();
    EXPECT(g_events_gone == 3 && live_count() == 41);
  }
  EXPECT(g_events_made == 44 && g_events_gone == 44 && live_count() == 0);
  {
    fh::Stream s;
    EXPECT((hipStream_t)s == nullptr);
    EXPECT(s.create(1u) == hipSuccess && ((hipStream_t)s)->flags == 1u && ((hipStream_t)s)->priority == 0 && live_count() == 1);
    EXPECT(s.create(1u, -1) == hipSuccess && ((hipStream_t)s)->priority == -1 && g_streams_made == 2 && g_streams_gone == 1);
    g_fail_after = 0;
    EXPECT(s.create(1u) == hipErrorOutOfMemory && (hipStream_t)s == nullptr && g_streams_gone == 2 && live_count() == 0);
    fh::Stream a, b;
    EXPECT(a.create(0u) == hipSuccess && b.create(0u) == hipSuccess);
    const hipStream_t ha = a;
    fh::Stream c(std::move(a));
    b = std::move(c);
    EXPECT((hipStream_t)b == ha && (hipStream_t)a == nullptr && (hipStream_t)c == nullptr && g_streams_gone == 3 && live_count() == 1);
    b.reset(); b.reset();
    EXPECT(g_streams_gone == 4);
  }
  EXPECT(g_streams_made == 4 && g_streams_gone == 4 && live_count() == 0 && live_bytes() == 0);
}

int main()
{
  check_buffer<fh::DeviceBuffer<uint32_t>>(0);
  check_buffer<fh::PinnedBuffer<uint32_t>>(1);
  EXPECT(g_allocs[0] == g_allocs[1] && g_allocs[0] > 0);  // (each kind went through its own pair of the seam)
  check_vector();
  check_handles();
  EXPECT(live_count() == 0 && live_bytes() == 0 && g_blocks[0].empty() && g_blocks[1].empty() && g_bad_frees == 0);
  if (failures) { std::printf("fh_memory_check: %d failures\n", failures); return 1; }
  std::printf("fh_memory_check: ok\n");
  return 0;
}
