// dev_arena.h -- the host plumbing around a handle's kernels: the layout of its one device block, the range test of a
// download, and the staging copies of a call's uploads.  Host code only.  The arena and the range test need no HIP (tests/cxx/
// dev_arena_test.cpp builds them with a plain compiler); what follows them wants cs_common.h included first.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

// A handle writes its layout ONCE, as a function that takes every array with its element count in the block's order, and runs it twice:
// over a null base for the byte total, over the allocation to bind the pointers.  Every array starts on a 256-byte boundary; a count of 0
// takes no room (the pointer is the next array's).
struct CsArena {
    char* base;   // null: the counting pass, no pointer is written
    size_t bytes = 0;
    explicit CsArena(void* b) : base((char*)b) {}
    template <typename T>
    void take(T*& p, size_t count) {
        if (base) p = (T*)(base + bytes);
        bytes += (count * sizeof(T) + 255) & ~(size_t)255;
    }
};

// n bytes at p lie inside [base, base + bytes): no sum that a huge n could wrap, a p below base becomes a huge offset
inline bool cs_arena_holds(const void* base, size_t bytes, const void* p, size_t n) {
    return n <= bytes && (size_t)((uintptr_t)p - (uintptr_t)base) <= bytes - n;
}

#ifdef CS_HIP

// count, allocate, zero, bind.  false: base is null and hipGetLastError() tells why.
template <typename Layout>
bool cs_arena_alloc(int device, char*& base, size_t& bytes, Layout layout) {
    CsArena count(nullptr);
    layout(count);
    bytes = count.bytes, base = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipMalloc((void**)&base, bytes) != hipSuccess) return false;
    if (hipMemset(base, 0, bytes) != hipSuccess) {
        (void)hipFree(base);
        base = nullptr;
        return false;
    }
    CsArena bind(base);
    layout(bind);
    return true;
}

// n bytes of a handle's block to the host; waits.  A null base (the caller had no handle) is refused with the rest.
inline int cs_arena_download(const char* who, int device, const char* base, size_t bytes, void* hip_stream, const void* d_src, void* h_dst,
                             size_t n) {
    if (!base || !d_src || !h_dst || !cs_arena_holds(base, bytes, d_src, n)) {
        cs_set_error("%s: the range is not inside the handle's buffers", who);
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(device));
    CS_HIP(hipMemcpyAsync(h_dst, d_src, n, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
    CS_HIP(hipStreamSynchronize((hipStream_t)hip_stream));
    return CS_OK;
}

// The host side of the uploads a call enqueues.  The copies are asynchronous, so a block stays alive until the NEXT call's begin, which
// waits for the stream the blocks were enqueued on -- the previous call's, whatever stream the new call runs on -- before it drops them.
struct CsStage {
    std::vector<std::vector<char>> blocks;
    hipStream_t stream = nullptr;
    int begin(hipStream_t s) {
        if (!blocks.empty()) {
            CS_HIP(hipStreamSynchronize(stream));
            blocks.clear();
        }
        stream = s;
        return CS_OK;
    }
    char* block(size_t bytes) {
        blocks.emplace_back(bytes);
        return blocks.back().data();
    }
    int upload(hipStream_t s, void* d_dst, const void* h_src, size_t bytes) {
        if (!bytes) return CS_OK;
        char* h = block(bytes);
        memcpy(h, h_src, bytes);
        CS_HIP(hipMemcpyAsync(d_dst, h, bytes, hipMemcpyHostToDevice, s));
        return CS_OK;
    }
    void drain() {   // before the handle's block is freed; the device, not the stream: the caller may have destroyed that by now
        (void)hipDeviceSynchronize();
        blocks.clear();
    }
};

#endif  // CS_HIP
