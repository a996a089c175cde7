// Stand-alone host check of gar_constrain's argument checks (include/gar_hip.h): every call below has to be refused with
// GAR_ERR_ARG and a message before anything is launched, so the program needs no GPU. Built with the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Igrasp-any-region_amd/csrc \
//       grasp-any-region_amd/csrc/constrain.hip grasp-any-region_amd/csrc/core.hip grasp-any-region_amd/csrc/llm.hip \
//       tools/constrain_host_check.cpp -o constrain_host_check && ./constrain_host_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/gar_hip.h"

static int failures = 0;

static void refused(const char* what, int rc, const char* needle) {
    const char* msg = gar_last_error();
    const bool ok = rc != 0 && msg && strstr(msg, needle);
    printf("%-46s rc %d  %s\n", what, rc, msg ? msg : "(no message)");
    if (!ok) {
        printf("  FAILED: expected a refusal that names \"%s\"\n", needle);
        ++failures;
    }
}

int main() {
    const int B = 2, V = 37, ld = 64, cols = 6;
    std::vector<float> logits((size_t)B * ld, 0.f);
    std::vector<int64_t> toks((size_t)B * cols, 0), eos = {2};
    std::vector<int32_t> trie = {1, 0, B, 0, 0, 0, 0, 0, 0}, nodes((size_t)B * (cols + 1), 0), step = {0};
    void* x = logits.data();
    const int tw = (int)trie.size();
    // the well-formed call would be (GAR_F32, x, ld, B, V, toks, cols, cols, step, eos, 1, trie, tw, nodes, cols + 1, 0)
    refused("dtype 7", gar_constrain(7, x, ld, B, V, toks.data(), cols, cols, step.data(), eos.data(), 1, trie.data(), tw, nodes.data(), cols + 1, 0), "dtype");
    refused("logits NULL", gar_constrain(GAR_F32, 0, ld, B, V, toks.data(), cols, cols, step.data(), eos.data(), 1, trie.data(), tw, nodes.data(), cols + 1, 0), "bad args");
    refused("trie NULL", gar_constrain(GAR_F32, x, ld, B, V, toks.data(), cols, cols, step.data(), eos.data(), 1, 0, tw, nodes.data(), cols + 1, 0), "bad args");
    refused("nodes NULL", gar_constrain(GAR_F32, x, ld, B, V, toks.data(), cols, cols, step.data(), eos.data(), 1, trie.data(), tw, 0, cols + 1, 0), "bad args");
    refused("B = 0", gar_constrain(GAR_F32, x, ld, 0, V, toks.data(), cols, cols, step.data(), eos.data(), 1, trie.data(), tw, nodes.data(), cols + 1, 0), "bad args");
    refused("V = 0", gar_constrain(GAR_F32, x, ld, B, 0, toks.data(), cols, cols, step.data(), eos.data(), 1, trie.data(), tw, nodes.data(), cols + 1, 0), "bad args");
    refused("ld < V", gar_constrain(GAR_F32, x, V - 1, B, V, toks.data(), cols, cols, step.data(), eos.data(), 1, trie.data(), tw, nodes.data(), cols + 1, 0), "bad args");
    refused("V above the bitmap", gar_constrain(GAR_BF16, x, (int64_t)1 << 20, B, gar_logits_process_max_vocab() + 1, toks.data(), cols, cols, step.data(), eos.data(), 1, trie.data(), tw, nodes.data(), cols + 1, 0), "above");
    refused("trie_words below the header", gar_constrain(GAR_F32, x, ld, B, V, toks.data(), cols, cols, step.data(), eos.data(), 1, trie.data(), 3, nodes.data(), cols + 1, 0), "header");
    refused("trie_words negative", gar_constrain(GAR_F32, x, ld, B, V, toks.data(), cols, cols, step.data(), eos.data(), 1, trie.data(), -5, nodes.data(), cols + 1, 0), "header");
    refused("out_cols negative", gar_constrain(GAR_F32, x, ld, B, V, toks.data(), cols, -1, step.data(), eos.data(), 1, trie.data(), tw, nodes.data(), cols + 1, 0), "out_cols");
    refused("out_stride below out_cols", gar_constrain(GAR_F32, x, ld, B, V, toks.data(), cols - 1, cols, step.data(), eos.data(), 1, trie.data(), tw, nodes.data(), cols + 1, 0), "out_stride");
    refused("node_stride = out_cols", gar_constrain(GAR_F32, x, ld, B, V, toks.data(), cols, cols, step.data(), eos.data(), 1, trie.data(), tw, nodes.data(), cols, 0), "node_stride");
    refused("node_stride 0 without tokens", gar_constrain(GAR_F32, x, ld, B, V, 0, 0, 0, 0, eos.data(), 1, trie.data(), tw, nodes.data(), 0, 0), "node_stride");
    refused("out_cols INT_MAX", gar_constrain(GAR_F32, x, ld, B, V, toks.data(), (int64_t)1 << 40, 0x7fffffff, step.data(), eos.data(), 1, trie.data(), tw, nodes.data(), 0x7fffffff, 0), "node_stride");
    refused("n_eos negative", gar_constrain(GAR_F32, x, ld, B, V, toks.data(), cols, cols, step.data(), eos.data(), -1, trie.data(), tw, nodes.data(), cols + 1, 0), "eos_ids");
    refused("eos_ids NULL with n_eos 1", gar_constrain(GAR_F32, x, ld, B, V, toks.data(), cols, cols, step.data(), 0, 1, trie.data(), tw, nodes.data(), cols + 1, 0), "eos_ids");
    printf(failures ? "%d checks FAILED\n" : "all refusals as specified (%d failed)\n", failures);
    return failures ? 1 : 0;
}
