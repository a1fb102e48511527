// The host transcript object behind bzh_transcript_* (csrc/transcript.hip); csrc/transcript_batch.hip reads and writes it in
// bzh_transcript_batch_from_host / _to_host.
#pragma once
#include <vector>

#include "blake2b.hpp"

struct bzh_transcript {
    bzh::Blake2b state;
    int field;
    std::vector<uint8_t> proof;
};
