// Host interface of the prime-search translation unit (engine_prime.hip): the launch of k_mr_w and the sieve.
// The C entry points pai_prime_test, pai_next_prime, pai_prime_last_times and pai_debug_prime_sieve (flexpai.h) are
// defined there too: they take no context.
#pragma once
#include <algorithm>
#include <vector>

#include "host_bignum.hpp"
#include "kernels_prime.hpp"

namespace fpai {

// k_mr_w<K> for candidates of `bits` bits (256, 512, 1024, 2048 -> K = 10, 19, 37, 74) over p.nwork work items;
// hipErrorInvalidValue for other sizes
hipError_t mr_launch(int bits, const prime::Params& p, hipStream_t st);

constexpr uint32_t PRIME_SIEVE_BOUND = 2000;   // _bigint._SMALL_PRIMES: trial division by the odd primes below it
constexpr int PRIME_MR_BASES = 40;             // _bigint.is_probable_prime: the first 40 odd primes

// x mod every odd prime below PRIME_SIEVE_BOUND, in the order of odd_small_primes()
const std::vector<uint32_t>& odd_small_primes();
std::vector<uint32_t> prime_residues(const HBig& x);
// the odd x + off, lo < off <= lo + window, that no odd prime below PRIME_SIEVE_BOUND divides (ascending offsets)
void prime_sieve_window(const HBig& x, const std::vector<uint32_t>& residues, uint32_t lo, uint32_t window,
                        std::vector<uint32_t>& offsets);

}  // namespace fpai
