// scoped_buffer.h — move-only owner of one allocation, freed in its destructor.
// Plain C++ (no HIP): the allocator is a policy, so the holder's move / release / destructor
// paths run on the host under a sanitizer (tests/scoped_buffer_driver.cpp).
//   Alloc::alloc(void **p, size_t bytes) -> status (0 = success)      Alloc::free(void *p)
#pragma once
#include <cstddef>
#include <utility>

namespace pupil {

template <typename T, typename Alloc>
class ScopedBuffer {
public:
    ScopedBuffer() = default;
    ScopedBuffer(const ScopedBuffer &) = delete;
    ScopedBuffer &operator=(const ScopedBuffer &) = delete;
    ScopedBuffer(ScopedBuffer &&o) noexcept : p_(o.release()) {}
    ScopedBuffer &operator=(ScopedBuffer &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.release();
        }
        return *this;
    }
    ~ScopedBuffer() { reset(); }

    // `count` entries (at least one); what the holder held before is freed first
    auto alloc(size_t count) {
        reset();
        void *p = nullptr;
        const auto status = Alloc::alloc(&p, sizeof(T) * (count > 0 ? count : 1));
        if (!status) p_ = static_cast<T *>(p);
        else if (p) Alloc::free(p);
        return status;
    }
    T *get() const { return p_; }
    // hands the allocation to the caller (a pointer that outlives the build)
    T *release() {
        T *p = p_;
        p_ = nullptr;
        return p;
    }
    void reset() {
        if (p_) Alloc::free(p_);
        p_ = nullptr;
    }

private:
    T *p_ = nullptr;
};

// The same for one handle (an event, a stream): Destroy::destroy(H) in the destructor.  Reads as
// the handle it holds; put() is where a create call writes a new one.
template <typename H, typename Destroy>
class ScopedHandle {
public:
    ScopedHandle() = default;
    explicit ScopedHandle(H h) : h_(h) {}
    ScopedHandle(ScopedHandle &&o) noexcept : h_(o.release()) {}
    ScopedHandle &operator=(ScopedHandle &&o) noexcept {
        if (this != &o) *put() = o.release();
        return *this;
    }
    ~ScopedHandle() { reset(); }

    operator H() const { return h_; }
    H *put() {
        reset();
        return &h_;
    }
    H release() { return std::exchange(h_, H{}); }
    void reset() {
        if (h_) Destroy::destroy(release());
    }

private:
    H h_{};
};

}  // namespace pupil
