// dev_buf.hpp -- who owns a ctx's device and pinned memory: ONE growable buffer type, the ledger behind
// rmx_scratch_bytes, and a buffer whose content is cached under a host-side key.  The grow-on-demand routine stands here
// once: a buffer that lets go of a block waits for the ctx's stream first, a failed request leaves "holds nothing,
// capacity 0", and a keyed buffer whose refill fails matches no key.
// No HIP in here: the memory calls come in through a policy type M --
//     void* alloc(size_t bytes) / void free(void*)                 device memory; alloc returns nullptr on failure
//     void* alloc_pinned(size_t bytes) / void free_pinned(void*)   pinned host memory, likewise
//     bool upload(void* dst, const void* src, size_t bytes)        host -> device, done on return
//     void wait()                                                  for the ctx's stream
//     void refused(const char* what, size_t bytes)                 a request that reserve / assign could not serve
// rmx_hip.hip instantiates it with the HIP calls, tests/host/test_dev_buf.cpp with a counting malloc that fails on demand
// (g++ -fsanitize=address,undefined, tests/test_dev_buf_sanitized.py).
#pragma once
#include <cstddef>
#include <utility>

namespace rmx {
namespace mem {

// what the buffers of one ctx share: the memory calls, and the bytes its counted buffers hold
template <class M>
struct Arena {
    M m;
    size_t ledger = 0;
};

enum Kind {
    kCounted,     // device memory that rmx_scratch_bytes reports
    kUncounted,   // device memory it does not
    kPinned       // pinned host memory (never counted)
};

// An owning buffer of `capacity()` elements T: move-only, freed in its destructor.  The destructor does NOT wait -- whoever
// destroys the ctx has waited for its stream --, everything else that lets go of a block does.
template <class T, class M, Kind K>
class Buf {
public:
    explicit Buf(Arena<M>* a) : a_(a) {}
    Buf(Buf&& o) noexcept : a_(o.a_), p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            release();
            a_ = o.a_;
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { drop(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }   // a buffer goes wherever its pointer went: kernel arguments, copies, null checks
    size_t capacity() const { return cap_; }
    size_t bytes() const { return cap_ * sizeof(T); }

    // room for n elements; the content does not survive a growth.  false: holds nothing (the caller copes: generic_ensure)
    bool try_reserve(size_t n) {
        if (n <= cap_) return true;
        release();
        p_ = static_cast<T*>(K == kPinned ? a_->m.alloc_pinned(n * sizeof(T)) : a_->m.alloc(n * sizeof(T)));
        if (!p_) return false;
        cap_ = n;
        if (K == kCounted) a_->ledger += bytes();
        return true;
    }
    // the same, and a failure is the call's: the policy hears of it
    bool reserve(size_t n) {
        if (try_reserve(n)) return true;
        a_->m.refused(K == kPinned ? "pinned allocation" : "device allocation", n * sizeof(T));
        return false;
    }
    // reserve + upload; a block that stays is waited for before it is overwritten.  false: holds nothing
    bool assign(const T* src, size_t n) {
        static_assert(K != kPinned, "assign uploads to the device");
        const bool stays = p_ && n <= cap_;
        if (!reserve(n)) return false;
        if (stays) a_->m.wait();
        if (n == 0 || a_->m.upload(p_, src, n * sizeof(T))) return true;
        release();
        a_->m.refused("upload", n * sizeof(T));
        return false;
    }
    template <class V>
    bool assign(const V& v) { return assign(v.data(), v.size()); }
    void release() {
        if (!p_) return;
        a_->m.wait();   // work in flight may still use the block
        drop();
    }

private:
    void drop() {
        if (!p_) return;
        if (K == kCounted) a_->ledger -= bytes();
        if (K == kPinned) a_->m.free_pinned(p_); else a_->m.free(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    Arena<M>* a_;
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// A device buffer whose content is cached under a host-side Key (==, default-constructible): holds(k) says whether a
// refill can be skipped.  The key is cleared BEFORE the block is touched and set only AFTER the upload has succeeded, so a
// refill that fails leaves a buffer that holds no key -- never a stale key over a block that was not filled.
template <class T, class M, class Key, Kind K = kUncounted>
class Keyed {
public:
    explicit Keyed(Arena<M>* a) : buf_(a) {}
    bool holds(const Key& k) const { return set_ && key_ == k; }
    T* get() const { return buf_.get(); }
    operator T*() const { return buf_.get(); }
    size_t capacity() const { return buf_.capacity(); }
    bool refill(const Key& k, const T* src, size_t n) {
        set_ = false;
        key_ = Key();
        if (!buf_.assign(src, n)) return false;
        key_ = k;
        set_ = true;
        return true;
    }
    template <class V>
    bool refill(const Key& k, const V& v) { return refill(k, v.data(), v.size()); }

private:
    Buf<T, M, K> buf_;
    Key key_{};
    bool set_ = false;
};

}  // namespace mem
}  // namespace rmx
