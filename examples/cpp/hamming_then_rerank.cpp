// hamming_then_rerank.cpp — two-stage retrieval over one MVF file with include/mvf.hpp: the fetch_k nearest rows of a UInt8
// space of bit-packed sign bits by Hamming distance (GpuVectorSpace::find_top_k_hamming), then those rows scored exactly on
// the Float32 space of the same file (GpuVectorSpace::rerank_top_k).
//
//   hamming_then_rerank <file.mvf> <binary space> <float space> <query row> <fetch_k> <k>
//
// The query is row <query row> of both spaces.  Prints one line per stage, `<name>: index:scorebits ...`, score bits in hex.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mvf.hpp"

static void print_hits(const char* name, const std::vector<mvf::ScoredVector>& hits) {
    std::printf("%s:", name);
    for (const auto& h : hits) {
        uint32_t bits;
        std::memcpy(&bits, &h.score, 4);
        std::printf(" %" PRIu64 ":%08x", h.index, bits);
    }
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: hamming_then_rerank <file.mvf> <binary space> <float space> <query row> <fetch_k> <k>\n");
        return 2;
    }
    try {
        const mvf::MvfReader reader = mvf::MvfReader::open(argv[1]);
        const mvf::VectorSpace bits = reader.vector_space(argv[2]), floats = reader.vector_space(argv[3]);
        const size_t row = (size_t)std::strtoull(argv[4], nullptr, 10);
        const size_t fetch_k = (size_t)std::strtoull(argv[5], nullptr, 10), k = (size_t)std::strtoull(argv[6], nullptr, 10);
        const auto packed = bits.get_vector(row).as_bytes();
        const std::vector<uint8_t> bq(packed.first, packed.first + packed.second);
        const std::vector<float> fq = floats.get_vector(row).as_f32();
        const mvf::GpuVectorSpace first(bits), second(floats);
        const std::vector<mvf::ScoredVector> coarse = first.find_top_k_hamming(bq, fetch_k);
        std::vector<uint64_t> candidates;
        for (const auto& h : coarse) candidates.push_back(h.index);
        print_hits("hamming", coarse);
        print_hits("reranked", second.rerank_top_k(fq, candidates, k));
    } catch (const mvf::MvfError& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
