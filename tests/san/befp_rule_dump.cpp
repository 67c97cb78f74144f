// befp_rule_dump.cpp — drives plan::befp_precheck (DESIGN §19, B1 and B2, and what the prep kernel of cda_befp_validate
// derives from a proof that passes them) over one call's arrays read from the file named on the command line:
//   k nproofs nentries nnodes_total nroots
//   nproofs lines   axis index entry_off nshares root_off
//   nentries lines  pos node_off nnodes <share: 1024 hex digits>
// and prints, per proof, "P <pre> <axis index>", then per slot j < 2k
//   "<start> <end> <node_off> <nnodes> <leaf_off> <root> <namespace hex> <mask>".
// tests/test_befp.py compares the lines with its Python restatement.  Host only: plan.cpp + this file, any C++17
// compiler; built with AddressSanitizer and UBSan by the test.  Every array is a std::vector of exactly the elements
// the file gives, so a read through an unbounded offset is an error there.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../celestia-app_amd/csrc/plan.h"

namespace {
int nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  uint32_t k = 0, nproofs = 0, nentries = 0, nnodes = 0, nroots = 0;
  if (!(in >> k >> nproofs >> nentries >> nnodes >> nroots)) return 2;
  std::vector<cda_befp_desc> descs(nproofs);
  std::vector<cda_befp_entry> entries(nentries);
  std::vector<uint8_t> shares((size_t)nentries * 512);
  for (auto& d : descs)
    if (!(in >> d.axis >> d.index >> d.entry_off >> d.nshares >> d.root_off)) return 2;
  for (uint32_t e = 0; e < nentries; e++) {
    std::string hex;
    if (!(in >> entries[e].pos >> entries[e].node_off >> entries[e].nnodes >> hex) || hex.size() != 1024) return 2;
    for (int i = 0; i < 512; i++) {
      const int a = nibble(hex[2 * i]), b = nibble(hex[2 * i + 1]);
      if (a < 0 || b < 0) return 2;
      shares[(size_t)e * 512 + i] = (uint8_t)(a * 16 + b);
    }
  }
  cda::plan::BefpPlan out;
  cda::plan::befp_precheck(k, nproofs, descs.data(), entries.data(), nentries, shares.data(), nnodes, nroots, out);
  const size_t w = 2 * (size_t)k;
  for (uint32_t p = 0; p < nproofs; p++) {
    printf("P %d %llu\n", out.pre[p], (unsigned long long)out.axis_index[p]);
    for (size_t j = 0; j < w; j++) {
      const cda_nmt_proof_desc& d = out.descs[p * w + j];
      printf("%u %u %u %u %u %u ", d.start, d.end, d.node_off, d.nnodes, d.leaf_off, d.root);
      for (int i = 0; i < 29; i++) printf("%02x", out.namespaces[(p * w + j) * 29 + i]);
      printf(" %u\n", out.mask[p * w + j]);
    }
  }
  return 0;
}
