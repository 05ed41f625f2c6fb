// neighbor_sum.h -- the one constant that the reductions over neighbour lists share (moments.hip,
// neighbor_reduce.hip): their rule cuts a list into blocks of kSum positions, sums every block from +0.0f in
// ascending position and adds the blocks' partials in block order.
#pragma once
#include <stdint.h>

namespace hidegs {

constexpr uint32_t kSum = 64;  // positions of a block of the rule

}  // namespace hidegs
