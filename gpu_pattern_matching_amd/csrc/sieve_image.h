// The tables of the sparse pipeline (sieve_tables.h) as the host builds them: plain vectors and the
// scalars the kernels get with them.  Host code only: acm_dfa_upload copies the vectors to the device
// as they are, acm_sieve_selftest looks everything up in them again without one.
#pragma once

#include <cstdint>
#include <vector>

#include "acm_internal.h"
#include "sieve_tables.h"

namespace acm {

struct SieveImage {
	bool applies = false;   // a set with patterns, none shorter than 3 bytes: the scalars below are set
	bool ok = false;        // ... and the edge index fits a record: the vectors are complete
	uint32_t W = 0, D = 0, LG = 0;          // stride, prefix length, bytes of a filter key (3 or 6)
	uint32_t run_ok[8] = { 0 };             // bit b: D copies of byte b are a trie path
	uint32_t bloom_log_words = 0;
	uint32_t gram_log_buckets = 0, gram_probes = 0;
	uint32_t prefix_log_slots = 0, prefix_probes = 0;
	uint32_t num_keys = 0, num_grams = 0;   // distinct filter keys, distinct 3-grams
	std::vector<uint32_t> bloom;            // [1 << bloom_log_words]
	std::vector<uint32_t> gram;             // [4 << gram_log_buckets]
	std::vector<uint32_t> prefix;           // [4 << prefix_log_slots]
	std::vector<SieveRec> rec, edges;       // [states], [edges + 1]
};

void build_sieve_image(const acm_automaton &a, SieveImage &img);

// the in_byte array as uploaded: [states + 224], device numbering
std::vector<uint8_t> device_in_byte(const acm_automaton &a);

}  // namespace acm
