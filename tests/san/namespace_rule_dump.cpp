// namespace_rule_dump.cpp — drives plan::namespace_bounds (ProveNamespace's rules P1-P3) and plan::namespace_precheck
// (VerifyNamespace's rules V1-V5) over cases read from stdin, one per line, hex without separators, "-" for nothing:
//   P <nid> <root> <nleaves> <leaf namespaces, 29 B each>            -> "<kind> <start> <end>"
//   V <nid> <start> <end> <nnodes> <nodes, 90 B each> <leaf_hash> <nleaves> <root>   -> "<0..3>"
// tests/test_namespace.py compares the lines with cda.wrapper / cda.proof (prove_namespace, verify_namespace).
// Host only: plan.cpp + this file, any C++17 compiler; built with AddressSanitizer and UBSan by the test.  Every
// buffer is a std::vector of exactly the bytes the line gives, so a read past a node or a namespace is an error there.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../celestia-app_amd/csrc/plan.h"

namespace {
int nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }
bool unhex(const std::string& s, std::vector<uint8_t>& out) {
  out.clear();
  if (s == "-") return true;
  if (s.size() % 2) return false;
  for (size_t i = 0; i < s.size(); i += 2) {
    const int a = nibble(s[i]), b = nibble(s[i + 1]);
    if (a < 0 || b < 0) return false;
    out.push_back((uint8_t)(a * 16 + b));
  }
  return true;
}
int fail(const std::string& line) {
  fprintf(stderr, "bad line: %.80s\n", line.c_str());
  return 2;
}
}  // namespace

int main() {
  std::string line;
  std::vector<uint8_t> nid, root, a, b;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string op, f0, f1, f2, f3;
    in >> op;
    if (op == "P") {
      unsigned nleaves = 0;
      if (!(in >> f0 >> f1 >> nleaves >> f2) || !unhex(f0, nid) || !unhex(f1, root) || !unhex(f2, a)) return fail(line);
      if (nid.size() != 29 || root.size() != 90 || a.size() != (size_t)nleaves * 29) return fail(line);
      const cda::plan::NamespaceBounds r = cda::plan::namespace_bounds(a.data(), 29, nleaves, root.data(), nid.data());
      printf("%u %u %u\n", r.kind, r.start, r.end);
    } else if (op == "V") {
      unsigned start = 0, end = 0, nnodes = 0, nleaves = 0;
      if (!(in >> f0 >> start >> end >> nnodes >> f1 >> f2 >> nleaves >> f3) || !unhex(f0, nid) || !unhex(f1, a) ||
          !unhex(f2, b) || !unhex(f3, root))
        return fail(line);
      if (nid.size() != 29 || root.size() != 90 || a.size() != (size_t)nnodes * 90 || (b.size() && b.size() != 90))
        return fail(line);
      printf("%d\n", cda::plan::namespace_precheck(nid.data(), start, end, a.data(), nnodes,
                                                   b.empty() ? nullptr : b.data(), nleaves, root.data()));
    } else {
      return fail(line);
    }
  }
  return 0;
}
