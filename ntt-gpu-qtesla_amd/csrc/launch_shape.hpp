// launch_shape.hpp -- the launch-shape rules of every chunked kernel of the
// library, in plain C++17 without a HIP include, so that a host-only program
// can compile and check them (tests/test_launch_shape.py).
#pragma once
#include <cstddef>
#include <cstdint>

namespace qntt {

struct LaunchShape {
    uint32_t grid, chunk;
};

constexpr size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// A workgroup takes `per` items per pass and walks `chunk` passes.  The chunk
// grows with the work (amortising the workgroup's prologue) but never beyond
// `max_chunk`, nor beyond what leaves `per_cu` workgroups for each of the
// `cus` compute units; the grid covers `items` with no workgroup left empty.
constexpr LaunchShape launch_shape(size_t items, size_t per, size_t cus, size_t per_cu, size_t max_chunk)
{
    size_t chunk = items / (per * cus * per_cu);
    chunk = chunk < 1 ? 1 : (chunk > max_chunk ? max_chunk : chunk);
    return {(uint32_t)ceil_div(items, per * chunk), (uint32_t)chunk};
}

// Grid of a kernel whose workgroups stride over the work: one workgroup per
// `wg` elements, at most `cap` per compute unit.
constexpr uint32_t capped_grid(size_t count, size_t wg, size_t cus, size_t cap)
{
    const size_t g = ceil_div(count, wg), m = cus * cap;
    return (uint32_t)(g < m ? g : m);
}

}  // namespace qntt
