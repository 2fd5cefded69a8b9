// Stand-alone host check of csrc/host/scoped_buffer.h (the BVH builder's device-scratch holder)
// with a counting allocator in place of hipMalloc / hipFree: every path must free each allocation
// exactly once.  Built with -fsanitize=address,undefined by test_scoped_buffer_host.py, so a
// double free, a leak or a use after free also fails the run by itself.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "host/scoped_buffer.h"

static std::set<void *> live;
static int allocs = 0, frees = 0, fail_at = -1;

struct CountingAlloc {
    static int alloc(void **p, size_t bytes) {
        if (allocs == fail_at) return 2;  // like hipErrorOutOfMemory: nothing allocated
        *p = std::malloc(bytes);
        live.insert(*p);
        allocs++;
        return 0;
    }
    static void free(void *p) {
        if (!live.erase(p)) {
            std::printf("FAIL free of a pointer that is not live\n");
            std::exit(1);
        }
        std::free(p);
        frees++;
    }
};
template <typename T>
using Buf = pupil::ScopedBuffer<T, CountingAlloc>;

static std::set<int *> open_handles;
static int created = 0, destroyed = 0;
static int *make_handle() {
    created++;
    return *open_handles.insert(new int(created)).first;
}
struct CountingDestroy {
    static void destroy(int *h) {
        if (!open_handles.erase(h)) {
            std::printf("FAIL destroy of a handle that is not open\n");
            std::exit(1);
        }
        delete h;
        destroyed++;
    }
};
using Handle = pupil::ScopedHandle<int *, CountingDestroy>;

#define CHECK(c)                                           \
    do {                                                   \
        if (!(c)) {                                        \
            std::printf("FAIL line %d: %s\n", __LINE__, #c); \
            return 1;                                      \
        }                                                  \
    } while (0)

template <typename T>
static Buf<T> scratch(int &err, size_t count) {  // bvh_build_detail.h scratch()
    Buf<T> b;
    if (!err) err = b.alloc(count);
    return b;
}

int main() {
    {  // destructor; a zero count still allocates one entry
        Buf<int> a;
        CHECK(a.get() == nullptr && a.alloc(0) == 0 && a.get() != nullptr);
        a.get()[0] = 7;
        Buf<double> b;
        CHECK(b.alloc(100) == 0);
        b.get()[99] = 1.0;
        CHECK(live.size() == 2);
    }
    CHECK(live.empty() && allocs == 2 && frees == 2);
    {  // move construction and move assignment over a holder that owns something
        Buf<int> a, c;
        CHECK(a.alloc(4) == 0 && c.alloc(8) == 0);
        int *pa = a.get();
        Buf<int> b(std::move(a));
        CHECK(a.get() == nullptr && b.get() == pa && live.size() == 2);
        c = std::move(b);  // frees c's own allocation
        CHECK(b.get() == nullptr && c.get() == pa && live.size() == 1);
        c = std::move(c);  // self-move keeps it
        CHECK(c.get() == pa && live.size() == 1);
        CHECK(c.alloc(2) == 0 && live.size() == 1);  // alloc over a live allocation frees it first
    }
    CHECK(live.empty() && allocs == frees);
    {  // release: the caller owns the pointer, the destructor leaves it alone
        int *kept = nullptr;
        {
            Buf<int> a;
            CHECK(a.alloc(3) == 0);
            kept = a.release();
            CHECK(a.get() == nullptr);
        }
        CHECK(live.size() == 1 && live.count(kept));
        kept[2] = 5;
        CountingAlloc::free(kept);
        Buf<int> e;
        CHECK(e.release() == nullptr);
        e.reset();
    }
    CHECK(live.empty() && allocs == frees);
    {  // an allocation sequence that fails midway: later ones are skipped, earlier ones freed
        fail_at = allocs + 2;
        int err = 0;
        auto a = scratch<int>(err, 10);
        auto b = scratch<char>(err, 10);
        auto c = scratch<float>(err, 10);
        auto d = scratch<int>(err, 10);
        CHECK(err == 2 && a.get() && b.get() && !c.get() && !d.get() && live.size() == 2);
        fail_at = -1;
    }
    CHECK(live.empty() && allocs == frees);
    {  // the handle holder (an event, a stream): destroyed once on every path
        Handle a, c;
        CHECK(!a && open_handles.empty());
        *a.put() = make_handle();
        *c.put() = make_handle();
        int *ha = a;
        Handle b(std::move(a));  // move construction
        CHECK(!a && b == ha && open_handles.size() == 2);
        c = std::move(b);  // move assignment over a held one destroys it
        CHECK(!b && c == ha && open_handles.size() == 1);
        c = std::move(c);  // self-move keeps it
        CHECK(c == ha && open_handles.size() == 1);
        *c.put() = make_handle();  // put over a held one destroys it first
        CHECK(open_handles.size() == 1 && !open_handles.count(ha));
        int *kept = c.release();  // release: the caller's to destroy
        CHECK(!c && open_handles.count(kept));
        c.reset();
        CountingDestroy::destroy(kept);
        Handle d(make_handle());  // destroyed with its scope
        CHECK(open_handles.size() == 1);
    }
    CHECK(open_handles.empty() && created == destroyed && created == 4);
    std::printf("ok %d allocations\n", allocs);
    return 0;
}
