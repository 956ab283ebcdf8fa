// arrow_c.hpp — the Arrow C Data Interface layer (arrow_c.cpp) as its two users see it: the device batch import / export in
// arrow_c.cpp itself and the IPC file writer / reader of ipc.cpp.
#pragma once
#include <memory>
#include <vector>

#include "core.hpp"

namespace bhip {

// Arrow C Data Interface format strings <-> bhip_dtype
int dtype_from_format(const char* fmt);
const char* format_of_dtype(int dt);

// `schema` as a struct ArrowSchema (LargeUtf8 / Binary fields under their boundary types)
void export_schema(const Schema& schema, ArrowSchema* out);

// bits [off, off + n) of `src` as a bitmap that starts at bit 0: whole zero-padded 64-bit words, 8 bytes to spare
std::vector<uint8_t> slice_bits(const uint8_t* src, int64_t off, int64_t n);

// One incoming Arrow array as plain host buffers of rows [0, n): the array's own `offset` (and its parent's) is taken out of every
// buffer.  O is the offset type of a variable-width array (int32_t: Utf8 / Binary, int64_t: LargeUtf8), unused otherwise.
// Nothing is copied but the bitmaps; what the consumer does with the parts (keep or drop the validity, narrow the offsets, write
// them in place) is the consumer's policy.
template <class O>
struct ArrowColumn {
    int64_t n = 0;
    bool has_validity = false;       // a validity buffer, and a null_count that does not rule NULLs out
    std::vector<uint8_t> validity;   // where has_validity
    int64_t null_count = 0;          // counted from `validity`
    std::vector<uint8_t> bits;       // Boolean: the values
    const O* offsets = nullptr;      // variable width: the array's offsets from row 0 on, as they are (first value `base`); null
    O base = 0;                      //   in an array of no rows that came without the buffer
    const void* data = nullptr;      // fixed width: row 0 on; variable width: byte `base` on (null where the array has no data buffer)
    int64_t data_bytes = 0;
    // out[0 .. n] = offsets[0 .. n] - base: n + 1 offsets that start at 0
    template <class T> void rebase_into(T* out) const {
        for (int64_t r = 0; r <= n; ++r) out[r] = offsets ? (T)(offsets[r] - base) : 0;
    }
};
// dt: DT_UTF8 for every variable-width type, DT_BOOLEAN, or a fixed-width type; `off`: the offset to apply (array + parents)
template <class O> ArrowColumn<O> normalise_array(const ArrowArray& a, int64_t off, int dt, const char* name);

// What an exported struct array (one RecordBatch) points to: the top-level array with its one (null) buffer, the children and their
// buffer lists, and whatever keeps the buffers alive.  The children own nothing: releasing the top-level array releases it all.
struct StructArrayShell {
    std::vector<ArrowArray> children;
    std::vector<ArrowArray*> child_ptrs;
    std::vector<std::vector<const void*>> buffers;       // per child
    const void* top_buffer = nullptr;
    std::vector<void*> owned;                            // malloc'd host buffers
    std::shared_ptr<void> owner;                         // or an object the buffers live in (an IPC file)
    explicit StructArrayShell(size_t n_children);
    ~StructArrayShell();
    void* alloc(size_t bytes);                           // a host buffer that lives as long as the array
    // child `i`: length n_rows, the buffers pushed into buffers[i] so far
    void finish_child(size_t i, int64_t n_rows, int64_t null_count);
    // hands `shell` over to *out
    static void finish(std::unique_ptr<StructArrayShell> shell, int64_t n_rows, ArrowArray* out);
};

}  // namespace bhip
