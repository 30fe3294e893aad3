// dev_arena_test.cpp -- the layout arena and the range test of coslam_amd/csrc/dev_arena.h on the host: a plain C++ compiler, no HIP.
// tests/test_mergefront_cpu.py builds and runs it; exit code 0 and "dev_arena ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../coslam_amd/csrc/dev_arena.h"

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)

struct Tables {
    int* a;             // 7 ints
    double* b;          // 100 doubles
    unsigned char* c;   // 0 bytes
    unsigned char* d;   // 257 bytes
    const float* e;     // 64 floats: 256 bytes exactly
    long long* f;       // 1
};

static void layout(Tables& t, CsArena& ar) {
    ar.take(t.a, 7), ar.take(t.b, 100), ar.take(t.c, 0), ar.take(t.d, 257), ar.take(t.e, 64), ar.take(t.f, 1);
}

int main() {
    // the counting pass: no pointer is written, the total is the sum of the arrays rounded up to 256 each
    Tables n = {};
    CsArena count(nullptr);
    layout(n, count);
    CHECK(count.bytes == 256 + 1024 + 0 + 512 + 256 + 256);
    CHECK(!n.a && !n.b && !n.c && !n.d && !n.e && !n.f);

    // the binding pass over an allocation of that size: the same total, aligned, in declared order, disjoint
    char* raw = (char*)malloc(count.bytes + 512);
    char* base = (char*)(((uintptr_t)raw + 255) & ~(uintptr_t)255) + 256;   // (room in front: base - 1 below is a pointer into raw)
    Tables t = {};
    CsArena bind(base);
    layout(t, bind);
    CHECK(bind.bytes == count.bytes);
    const char* p[6] = {(char*)t.a, (char*)t.b, (char*)t.c, (char*)t.d, (const char*)t.e, (char*)t.f};
    const size_t bytes[6] = {7 * sizeof(int), 100 * sizeof(double), 0, 257, 64 * sizeof(float), sizeof(long long)};
    CHECK(p[0] == base);
    for (int k = 0; k < 6; ++k) {
        CHECK(((uintptr_t)p[k] & 255) == 0);
        CHECK(cs_arena_holds(base, bind.bytes, p[k], bytes[k]));
        if (k + 1 < 6) CHECK(p[k] + bytes[k] <= p[k + 1]);   // ascending and disjoint
    }
    CHECK(p[5] + bytes[5] <= base + bind.bytes);
    CHECK(p[2] == p[3]);   // the zero-length array took no room: its pointer is the next array's
    for (size_t i = 0; i < count.bytes; ++i) base[i] = 0;   // every byte of the block is the caller's to write
    t.a[6] = 1, t.b[99] = 2.0, t.d[256] = 3, t.f[0] = 4;
    CHECK(t.a[6] == 1 && t.b[99] == 2.0 && t.d[256] == 3 && t.e[63] == 0.0f && t.f[0] == 4);

    // a layout of nothing but empty arrays
    Tables z = {};
    CsArena none(base);
    none.take(z.a, 0), none.take(z.b, 0);
    CHECK(none.bytes == 0 && (char*)z.a == base && (char*)z.b == base);

    // the range test
    const size_t B = bind.bytes;
    CHECK(cs_arena_holds(base, B, base, B));               // first byte to last byte
    CHECK(cs_arena_holds(base, B, base, 0));
    CHECK(cs_arena_holds(base, B, base + B - 1, 1));       // the last byte alone
    CHECK(cs_arena_holds(base, B, base + B, 0));           // nothing, at the end
    CHECK(!cs_arena_holds(base, B, base, B + 1));          // one byte past the end
    CHECK(!cs_arena_holds(base, B, base + 1, B));
    CHECK(!cs_arena_holds(base, B, base + B, 1));
    CHECK(!cs_arena_holds(base, B, base - 1, 1));          // a pointer before the base
    CHECK(!cs_arena_holds(base, B, base - 1, 0));
    CHECK(!cs_arena_holds(base, B, nullptr, 1));
    CHECK(!cs_arena_holds(base, B, base, SIZE_MAX));       // n > bytes
    CHECK(!cs_arena_holds(base, B, base + 16, SIZE_MAX));        // p + n wraps to p - 1
    CHECK(!cs_arena_holds(base, B, base + 16, SIZE_MAX - 15));   // p + n wraps to base exactly
    CHECK(!cs_arena_holds(base, 0, base, 1));
    free(raw);
    printf("dev_arena ok\n");
    return 0;
}
