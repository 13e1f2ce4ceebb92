// rerank_documents.cpp — late-interaction retrieval over an MVF file with include/mvf.hpp: the k best documents for a query of
// several vectors (GpuVectorSpace::find_top_k_documents), then the same query re-ranked among candidate documents only
// (GpuVectorSpace::rerank_top_k_documents), as behind a first-stage retriever.
//
//   rerank_documents <file.mvf> <space> <column> <n_tokens> <k> [candidate ...]
//
// The query is the space's first n_tokens vectors.  Prints one line per call, `<name>: key:scorebits ...`, score bits in hex.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mvf.hpp"

static void print_hits(const char* name, const std::vector<std::pair<uint64_t, float>>& hits) {
    std::printf("%s:", name);
    for (const auto& h : hits) {
        uint32_t bits;
        std::memcpy(&bits, &h.second, 4);
        std::printf(" %" PRIu64 ":%08x", h.first, bits);
    }
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: rerank_documents <file.mvf> <space> <column> <n_tokens> <k> [candidate ...]\n");
        return 2;
    }
    try {
        const mvf::MvfReader reader = mvf::MvfReader::open(argv[1]);
        const mvf::VectorSpace space = reader.vector_space(argv[2]);
        const mvf::MetadataColumn column = reader.metadata_column(argv[3]);
        const size_t n_tokens = (size_t)std::strtoull(argv[4], nullptr, 10), k = (size_t)std::strtoull(argv[5], nullptr, 10);
        std::vector<float> query;
        for (size_t t = 0; t < n_tokens; t++) {
            const std::vector<float> v = space.get_vector(t).as_f32();
            query.insert(query.end(), v.begin(), v.end());
        }
        std::vector<uint64_t> candidates;
        for (int i = 6; i < argc; i++) candidates.push_back(std::strtoull(argv[i], nullptr, 10));
        const mvf::GpuVectorSpace gpu(space);
        print_hits("documents", gpu.find_top_k_documents(query, k, column));
        print_hits("reranked", gpu.rerank_top_k_documents(query, candidates, k, column));
        print_hits("no candidates", gpu.rerank_top_k_documents(query, {}, k, column));
    } catch (const mvf::MvfError& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
