// TEST INFRASTRUCTURE — a host-only stand-in for <rocprim/rocprim.hpp>, for
// exactly what the blob builder (sview-fmindex_amd/csrc/fmx_build.hip) calls:
// double_buffer, radix_sort_pairs (the double_buffer overload),
// inclusive_scan with maximum<T> / plus<T>, and select with a flag array and
// a device count.  Written from rocPRIM's documented interface, and as
// unforgiving as that interface allows:
//   * a call with a null temporary buffer reports a non-zero size and does
//     nothing else; a real call with less storage than that is an error;
//   * a real call is queued on its stream (simt::submit_launch): under
//     deferred streams it runs later, in stream order, and reads its inputs
//     and the temporary storage when it runs, not when it is queued — a
//     buffer freed, reused or not yet written by then gives wrong bytes;
//   * the sort is stable and compares bits [begin_bit, end_bit) only; which
//     of the two buffers is current afterwards is drawn from the emulator's
//     seeded random stream (the double_buffer says so when the call returns,
//     as rocPRIM's does), the other buffer and the temporary storage end up
//     full of random bytes;
//   * select writes the selected elements and the count, nothing past them;
//     the scans write `size` elements.
// Not a product path: only tests/simt compiles against it.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace rocprim {

template <class T>
class double_buffer {
    T *buffers[2];
    unsigned selector;

  public:
    double_buffer() : buffers{nullptr, nullptr}, selector(0) {}
    double_buffer(T *current, T *alternate) : buffers{current, alternate}, selector(0) {}
    T *current() const { return buffers[selector]; }
    T *alternate() const { return buffers[selector ^ 1]; }
    void swap() { selector ^= 1; }
};

template <class T>
struct maximum {
    constexpr T operator()(const T &a, const T &b) const { return a < b ? b : a; }
};
template <class T>
struct plus {
    constexpr T operator()(const T &a, const T &b) const { return a + b; }
};

namespace shim_detail {
// what a size query reports: never zero, 256-byte granules, growing with the input
inline size_t storage_for(size_t size, size_t elem) { return 256 + ((size * elem / 8 + 255) & ~size_t(255)); }
}  // namespace shim_detail

template <class Key, class Value, class Size>
inline hipError_t radix_sort_pairs(void *temporary_storage, size_t &storage_size, double_buffer<Key> &keys,
                                   double_buffer<Value> &values, Size size, unsigned begin_bit = 0,
                                   unsigned end_bit = 8 * sizeof(Key), hipStream_t stream = 0, bool = false) {
    const size_t need = shim_detail::storage_for((size_t)size, sizeof(Key) + sizeof(Value));
    if (temporary_storage == nullptr) {
        storage_size = need;
        return hipSuccess;
    }
    if (storage_size < need || begin_bit >= end_bit || end_bit > 8 * sizeof(Key)) return hipErrorInvalidValue;
    Key *k_in = keys.current(), *k_alt = keys.alternate();
    Value *v_in = values.current(), *v_alt = values.alternate();
    // decided on the host, as rocPRIM decides it from the number of passes
    const bool flip = (::simt::host_random() & 1) != 0;
    if (flip) {
        keys.swap();
        values.swap();
    }
    const size_t m = (size_t)size, tmp_bytes = storage_size;
    return ::simt::submit_launch(stream, [=]() {
        const unsigned bits = end_bit - begin_bit;
        const Key mask = bits >= 8 * sizeof(Key) ? ~Key(0) : (Key)((Key(1) << bits) - 1);
        std::vector<size_t> order(m);
        std::iota(order.begin(), order.end(), size_t(0));
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
            return ((k_in[a] >> begin_bit) & mask) < ((k_in[b] >> begin_bit) & mask);
        });
        std::vector<Key> ks(m);
        std::vector<Value> vs(m);
        for (size_t j = 0; j < m; ++j) {
            ks[j] = k_in[order[j]];
            vs[j] = v_in[order[j]];
        }
        Key *k_out = flip ? k_alt : k_in, *k_junk = flip ? k_in : k_alt;
        Value *v_out = flip ? v_alt : v_in, *v_junk = flip ? v_in : v_alt;
        ::simt::host_fill_random(k_junk, m * sizeof(Key));
        ::simt::host_fill_random(v_junk, m * sizeof(Value));
        ::simt::host_fill_random(temporary_storage, tmp_bytes);
        std::copy(ks.begin(), ks.end(), k_out);
        std::copy(vs.begin(), vs.end(), v_out);
        return hipSuccess;
    });
}

template <class T, class BinaryFunction>
inline hipError_t inclusive_scan(void *temporary_storage, size_t &storage_size, const T *input, T *output, size_t size,
                                 BinaryFunction scan_op = BinaryFunction(), hipStream_t stream = 0, bool = false) {
    const size_t need = shim_detail::storage_for(size, sizeof(T));
    if (temporary_storage == nullptr) {
        storage_size = need;
        return hipSuccess;
    }
    if (storage_size < need) return hipErrorInvalidValue;
    const size_t tmp_bytes = storage_size;
    return ::simt::submit_launch(stream, [=]() {
        ::simt::host_fill_random(temporary_storage, tmp_bytes);
        if (size) {
            T acc = input[0];
            output[0] = acc;
            for (size_t j = 1; j < size; ++j) {
                acc = scan_op(acc, input[j]);
                output[j] = acc;
            }
        }
        return hipSuccess;
    });
}
template <class T, class BinaryFunction>
inline hipError_t inclusive_scan(void *temporary_storage, size_t &storage_size, T *input, T *output, size_t size,
                                 BinaryFunction scan_op = BinaryFunction(), hipStream_t stream = 0, bool = false) {
    return inclusive_scan(temporary_storage, storage_size, (const T *)input, output, size, scan_op, stream);
}

template <class T, class Flag, class Count>
inline hipError_t select(void *temporary_storage, size_t &storage_size, const T *input, const Flag *flags, T *output,
                         Count *selected_count_output, size_t size, hipStream_t stream = 0, bool = false) {
    const size_t need = shim_detail::storage_for(size, sizeof(T));
    if (temporary_storage == nullptr) {
        storage_size = need;
        return hipSuccess;
    }
    if (storage_size < need) return hipErrorInvalidValue;
    const size_t tmp_bytes = storage_size;
    return ::simt::submit_launch(stream, [=]() {
        ::simt::host_fill_random(temporary_storage, tmp_bytes);
        size_t count = 0;
        for (size_t j = 0; j < size; ++j)
            if (flags[j]) output[count++] = input[j];
        *selected_count_output = (Count)count;
        return hipSuccess;
    });
}
template <class T, class Flag, class Count>
inline hipError_t select(void *temporary_storage, size_t &storage_size, T *input, const Flag *flags, T *output,
                         Count *selected_count_output, size_t size, hipStream_t stream = 0, bool = false) {
    return select(temporary_storage, storage_size, (const T *)input, flags, output, selected_count_output, size,
                  stream);
}

}  // namespace rocprim
