// grow_buf.h -- the one grow-only buffer type behind every scratch allocation
// the host shim owns (host-only; the memory source is a policy, so this header
// needs no HIP header and is checked on the CPU by
// tests/integration/grow_buf_check.cpp over a policy that keeps a ledger).
//
// A policy M supplies
//     static bool alloc(size_t bytes, mcrc::Block *b);  // false: out of memory
//     static void free(const mcrc::Block &b);
// and does the source's own housekeeping on failure (the HIP policies clear
// the pending error, so it is not left for a later launch check).
#pragma once
#include <stddef.h>

namespace mcrc {

// One allocation: the address the host holds and the address kernels use
// (device memory: the same; page-locked memory that is not mapped: null).
struct Block {
    void *p = nullptr;
    void *dv = nullptr;
};

// reserve(bytes): the block when it already holds that many bytes (no
// allocator call); else the old block is freed, once, and exactly `bytes` are
// allocated.  When that fails the buffer is empty (null, 0 bytes), reserve
// returns null and a later reserve starts clean: no address that was freed is
// kept anywhere.  reserve(0) is the current block, possibly null.
//
// Not copyable, and no destructor frees: the buffers live in objects of
// static storage (the shim's device table), where a freeing destructor would
// call into the HIP runtime during static destruction.  Nothing is freed at
// process exit.
template <class M, class T = void>
class GrowBuf {
  public:
    GrowBuf() = default;
    GrowBuf(const GrowBuf &) = delete;
    GrowBuf &operator=(const GrowBuf &) = delete;

    T *reserve(size_t bytes) {
        if (bytes <= bytes_) return get();
        const Block old = b_;
        b_ = Block{};
        bytes_ = 0;
        if (old.p) M::free(old);
        Block nb;
        if (!M::alloc(bytes, &nb) || !nb.p) return nullptr;  // (whatever alloc left in nb is dropped)
        b_ = nb;
        bytes_ = bytes;
        return get();
    }
    T *get() const { return static_cast<T *>(b_.p); }
    T *dev() const { return static_cast<T *>(b_.dv); }  // the address kernels use
    size_t bytes() const { return bytes_; }

  private:
    Block b_;
    size_t bytes_ = 0;
};

}  // namespace mcrc
