// align_documents.cpp — which passage of each document matched which query token, with include/mvf.hpp: the late-interaction
// alignments of listed documents (GpuVectorSpace::align_documents), as behind find_top_k_documents or rerank_top_k_documents.
//
//   align_documents <file.mvf> <space> <column> <n_tokens> [key ...]
//
// The query is the space's first n_tokens vectors.  Prints one line per listed key, `<key>: row:scorebits ...`, one pair per
// token, score bits in hex.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mvf.hpp"

int main(int argc, char** argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: align_documents <file.mvf> <space> <column> <n_tokens> [key ...]\n");
        return 2;
    }
    try {
        const mvf::MvfReader reader = mvf::MvfReader::open(argv[1]);
        const mvf::VectorSpace space = reader.vector_space(argv[2]);
        const mvf::MetadataColumn column = reader.metadata_column(argv[3]);
        const size_t n_tokens = (size_t)std::strtoull(argv[4], nullptr, 10);
        std::vector<float> query;
        for (size_t t = 0; t < n_tokens; t++) {
            const std::vector<float> v = space.get_vector(t).as_f32();
            query.insert(query.end(), v.begin(), v.end());
        }
        std::vector<uint64_t> keys;
        for (int i = 5; i < argc; i++) keys.push_back(std::strtoull(argv[i], nullptr, 10));
        const mvf::GpuVectorSpace gpu(space);
        const auto aligned = gpu.align_documents(query, keys, column);
        for (size_t i = 0; i < keys.size(); i++) {
            std::printf("%" PRIu64 ":", keys[i]);
            for (const auto& hit : aligned[i]) {
                uint32_t bits;
                std::memcpy(&bits, &hit.second, 4);
                std::printf(" %" PRIu64 ":%08x", hit.first, bits);
            }
            std::printf("\n");
        }
    } catch (const mvf::MvfError& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
