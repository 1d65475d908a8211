// DevBuf (csrc/sns_devbuf.h) over a CPU allocator: the two allocator functions the library defines over hipMalloc / hipFree are
// malloc / free with a byte counter here, so ownership is checked without a GPU, under AddressSanitizer with leak detection.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <utility>
#include <vector>

#include "sns_devbuf.h"

static long long g_live = 0;
static bool g_fail = false;

namespace sns {
int dev_malloc_bytes(void** p, size_t bytes) {
    *p = nullptr;
    if (g_fail) return SNS_E_HIP;
    *p = std::malloc(bytes);
    if (!*p) return SNS_E_HIP;
    g_live += (long long)bytes;
    return SNS_OK;
}
void dev_free_bytes(void* p, size_t bytes) {
    std::free(p);
    g_live -= (long long)bytes;
}
int dev_upload_bytes(void* dst, const void* src, size_t bytes) {
    std::memcpy(dst, src, bytes);
    return SNS_OK;
}
}  // namespace sns
using sns::DevBuf;

static int g_bad = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_bad; } \
    } while (0)

struct Node {                                    // a struct of owners, as Level is
    int id = 0;
    DevBuf<double> x, b;
    DevBuf<void> bytes;
};

int main() {
    {
        DevBuf<double> a;
        CHECK(a.get() == nullptr && !a && a.count() == 0 && g_live == 0);
        CHECK(a.alloc(10) == SNS_OK && a && a.count() == 10 && g_live == 80);
        double* first = a;
        first[9] = 1.0;
        CHECK(a.alloc(20) == SNS_OK && a.count() == 20 && g_live == 160);          // alloc twice: the first allocation is freed
        CHECK(a.alloc(0) == SNS_OK && a.count() == 1 && g_live == 8);              // 0 means 1 element
        a.reset();
        CHECK(!a && a.count() == 0 && g_live == 0);
        a.reset();                                                                  // (idempotent)
        CHECK(g_live == 0);
    }
    {
        DevBuf<void> v;                                                             // sized in bytes
        CHECK(v.alloc(100) == SNS_OK && v.count() == 100 && g_live == 100);
        void* raw = v;
        CHECK(raw == v.get());
    }
    CHECK(g_live == 0);
    {
        std::vector<int> h = {1, 2, 3, 4, 5};
        DevBuf<int> d;
        CHECK(d.upload(h) == SNS_OK && d.count() == 5 && d[4] == 5 && g_live == 20);
        CHECK(d.upload(std::vector<int>()) == SNS_OK && d.count() == 1 && g_live == 4);
    }
    CHECK(g_live == 0);
    {
        DevBuf<double> a, c;
        CHECK(a.alloc(4) == SNS_OK && c.alloc(6) == SNS_OK && g_live == 80);
        double* pa = a;
        DevBuf<double> b(std::move(a));                                             // move construction: the source is empty
        CHECK(!a && a.count() == 0 && b.get() == pa && b.count() == 4 && g_live == 80);
        c = std::move(b);                                                           // move assignment: the target's 48 bytes are freed
        CHECK(!b && c.get() == pa && c.count() == 4 && g_live == 32);
        DevBuf<double>& alias = c;
        c = std::move(alias);                                                       // self-move: harmless
        CHECK(c.get() == pa && c.count() == 4 && g_live == 32);
    }
    CHECK(g_live == 0);
    {
        std::vector<DevBuf<double>> v;                                              // growth moves the owners
        std::vector<double*> raw;
        for (int i = 0; i < 100; ++i) {
            v.emplace_back();
            CHECK(v.back().alloc((size_t)i + 1) == SNS_OK);
            raw.push_back(v.back());
        }
        CHECK(g_live == 8LL * 100 * 101 / 2);
        for (int i = 0; i < 100; ++i) CHECK(v[(size_t)i].get() == raw[(size_t)i] && v[(size_t)i].count() == (size_t)i + 1);
        v.erase(v.begin() + 10, v.begin() + 20);
        long long gone = 0;
        for (int i = 10; i < 20; ++i) gone += 8LL * (i + 1);
        CHECK(g_live == 8LL * 100 * 101 / 2 - gone);
    }
    CHECK(g_live == 0);
    {
        std::deque<Node> d;                                                         // grows while a reference is live
        d.emplace_back();
        Node& first = d.front();
        CHECK(first.x.alloc(3) == SNS_OK && first.bytes.alloc(7) == SNS_OK);
        double* px = first.x;
        for (int i = 1; i < 200; ++i) {
            d.emplace_back();
            d.back().id = i;
            CHECK(d.back().x.alloc(2) == SNS_OK && d.back().b.alloc(2) == SNS_OK);
        }
        CHECK(&first == &d.front() && first.x.get() == px && first.x.count() == 3);
        CHECK(g_live == 24 + 7 + 199LL * 32);
        Node moved(std::move(d[5]));                                                // the struct is movable, not copyable
        CHECK(!d[5].x && !d[5].b && moved.x.count() == 2 && g_live == 24 + 7 + 199LL * 32);
        d.pop_back();
        CHECK(g_live == 24 + 7 + 198LL * 32);
    }
    CHECK(g_live == 0);
    {
        DevBuf<double> a;
        CHECK(a.alloc(5) == SNS_OK);
        g_fail = true;                                                              // the allocator reports failure
        CHECK(a.alloc(9) == SNS_E_HIP && !a && a.count() == 0 && g_live == 0);
        CHECK(a.upload(std::vector<double>(3, 1.0)) == SNS_E_HIP && !a && g_live == 0);
        g_fail = false;
        CHECK(a.alloc(2) == SNS_OK && g_live == 16);
    }
    CHECK(g_live == 0);
    static_assert(!std::is_copy_constructible<DevBuf<int>>::value && !std::is_copy_assignable<DevBuf<int>>::value, "move-only");
    static_assert(!std::is_copy_constructible<Node>::value && std::is_nothrow_move_constructible<Node>::value, "move-only struct");
    std::printf("devbuf: %s, live bytes at exit %lld\n", g_bad ? "FAILED" : "ok", g_live);
    return (g_bad || g_live != 0) ? 1 : 0;
}
