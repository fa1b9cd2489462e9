// surround_check.cpp — csrc/host/keyframe_select.h's surround_update as a stand-alone program, built by
// tests/test_surround_host.py with -fsanitize=address,undefined: the rule erases from the vector it walks.
// Input: one case per line, "<list ids> | <ds ids>"; output: the list afterwards, one line per case.
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "host/keyframe_select.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::vector<int> list, ds;
    std::istringstream in(line);
    std::string tok;
    bool right = false;
    while (in >> tok) {
      if (tok == "|")
        right = true;
      else
        (right ? ds : list).push_back(std::stoi(tok));
    }
    lins_select::surround_update(list, ds);
    for (size_t i = 0; i < list.size(); ++i) std::cout << (i ? " " : "") << list[i];
    std::cout << "\n";
  }
  return 0;
}
