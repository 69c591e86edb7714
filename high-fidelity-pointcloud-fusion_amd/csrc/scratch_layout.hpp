// csrc/scratch_layout.hpp -- one buffer cut into typed arrays.  Host only and free of HIP, so g++ alone compiles it
// (tests/scratch_layout_check.cpp).
//
// A caller declares its arrays once, in order: add(&ptr, count) for `count` elements of *ptr's type.  bytes() is then the size to
// allocate and place(base) sets every declared pointer, so the size and the offsets cannot disagree.  The pointers exist only after
// place(): a buffer that may move when it grows is cut after its allocation, never before.
#pragma once

#include <cstddef>
#include <cstdint>

namespace hfpf {

class ScratchLayout {
  public:
    // The next array: it starts at the next multiple of alignof(T) and takes count * sizeof(T) bytes, rounded up to a multiple of
    // `round_to` where the consumer wants whole lines (a power of two is not required).
    template <typename T>
    ScratchLayout& add(T** ptr, uint64_t count, uint64_t round_to = 1)
    {
        total_ = (total_ + alignof(T) - 1) / alignof(T) * alignof(T);
        if (n_ < kMaxSlices) slice_[n_] = Slice{ptr, total_, [](void* to, char* at) { *static_cast<T**>(to) = reinterpret_cast<T*>(at); }};
        n_++;
        total_ += (count * sizeof(T) + round_to - 1) / round_to * round_to;
        return *this;
    }
    // Bytes that belong to no array (room a consumer keeps behind the last one).
    ScratchLayout& skip(uint64_t bytes)
    {
        total_ += bytes;
        return *this;
    }
    uint64_t bytes() const { return total_; }
    bool fits() const { return n_ <= kMaxSlices; }  // false: more arrays declared than a layout holds (a static property of the caller)
    // base: an allocation of at least bytes() bytes, aligned for every declared type.
    void place(void* base) const
    {
        for (int i = 0; i < n_ && i < kMaxSlices; i++) slice_[i].set(slice_[i].ptr, static_cast<char*>(base) + slice_[i].off);
    }

  private:
    static constexpr int kMaxSlices = 8;
    struct Slice {
        void* ptr;
        uint64_t off;
        void (*set)(void*, char*);
    };
    Slice slice_[kMaxSlices] = {};
    int n_ = 0;
    uint64_t total_ = 0;
};

}  // namespace hfpf
