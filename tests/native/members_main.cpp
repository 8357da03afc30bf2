// Test-only driver of the resident-member bookkeeping (grandine_amd/csrc/gbls_members.h), a
// stand-alone program for ASan/UBSan: reads one operation per line from stdin, applies it with the
// call sequences gbls_capi.hip uses, keeps each block's indices in a heap vector of its own that is
// destroyed when the table hands the block out as dead (so a view into a freed block is a
// sanitizer report), and prints the whole state after every step for tests/test_bits_members.py
// to compare with its model.  Not part of the product.
//
//   M first ncom len...        gbls_committees_set_members (member k of the call's committee c is
//                              call * 65536 + its position in the call)
//   J first ncom len... mask   ... whose committee c comes back with a nonzero status when bit
//                              c % 32 of mask is set: those slots keep no members
//   P first ncom               gbls_committees_set
//   C                          gbls_committees_clear
//   R                          gbls_registry_set below the registry size
//   F first ncom len... members  a set call (members = 0 / 1) that fails before its slots are
//                              written: the table is truncated to first
//   V slot                     a reader resolves the slot and reads its members
//
// Output per step: "bytes=B peak=K blocks=N freed=<calls> | slot:len:v,v,... ..." with `freed` the
// calls whose blocks were handed out by this step and `peak` the bytes held inside the step.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <sstream>
#include <string>
#include <iostream>
#include <vector>

#include "../../grandine_amd/csrc/gbls_members.h"

using gbls::members::kNoBlock;
using gbls::members::Table;
using gbls::members::View;

struct Store {
  std::vector<uint32_t> *idx = nullptr;
  uint32_t call = 0;
};

int main() {
  Table tab;
  std::map<uint32_t, Store> store;  // block id -> its "device memory"
  size_t nslots = 0;
  uint32_t call = 0;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    char op;
    in >> op;
    size_t peak = tab.bytes_held();
    std::vector<uint32_t> freed;
    auto reap = [&]() {
      peak = std::max(peak, tab.bytes_held());
      for (uint32_t b : tab.take_dead()) {
        auto it = store.find(b);
        if (it == store.end()) {
          std::printf("ERROR dead block %u unknown or handed out twice\n", b);
          return false;
        }
        freed.push_back(it->second.call);
        delete it->second.idx;
        store.erase(it);
      }
      return true;
    };
    if (op == 'M' || op == 'J' || op == 'F') {
      size_t first, ncom;
      in >> first >> ncom;
      std::vector<uint32_t> off(ncom + 1, 0);
      for (size_t c = 0; c < ncom; c++) {
        uint32_t len;
        in >> len;
        off[c + 1] = off[c] + len;
      }
      uint32_t extra = 0;
      if (op != 'M') in >> extra;  // J: the rejected committees; F: whether the call keeps members
      call++;
      const bool keep = op != 'F' || extra;
      uint32_t blk = kNoBlock;
      uint64_t serial = 0;
      if (keep && ncom) {
        blk = tab.open_block(off[ncom]);
        serial = tab.serial(blk);
        if (store.count(blk)) {
          std::printf("ERROR block id %u reused while held\n", blk);
          return 1;
        }
        Store s;
        s.idx = new std::vector<uint32_t>(off[ncom]);
        s.call = call;
        for (uint32_t k = 0; k < off[ncom]; k++) (*s.idx)[k] = call * 65536u + k;
        store[blk] = s;
      }
      if (op == 'F') {  // the failure path of committees_set_impl
        if (blk != kNoBlock) tab.close_block(blk);
        tab.drop_from(first);
        nslots = std::min(nslots, first);
      } else {
        nslots = std::max(nslots, first + ncom);
        for (size_t c = 0; c < ncom; c++) tab.assign(first + c, blk, off[c], off[c + 1] - off[c]);
        if (blk != kNoBlock) tab.close_block(blk);
      }
      if (!reap()) return 1;
      if (op == 'J') {  // the statuses arrive after the lock was released
        for (size_t c = 0; c < ncom; c++)
          if ((extra >> (c % 32)) & 1) tab.drop_if(first + c, blk, serial);
        if (!reap()) return 1;
      }
    } else if (op == 'P') {
      size_t first, ncom;
      in >> first >> ncom;
      call++;
      nslots = std::max(nslots, first + ncom);
      for (size_t c = 0; c < ncom; c++) tab.drop(first + c);
      if (!reap()) return 1;
    } else if (op == 'C' || op == 'R') {
      tab.drop_from(0);
      nslots = 0;
      if (!reap()) return 1;
    } else if (op == 'V') {
      size_t slot;
      in >> slot;
    } else {
      std::printf("ERROR unknown operation %c\n", op);
      return 1;
    }
    size_t held = 0;
    for (auto &kv : store) held += kv.second.idx->size() * 4;
    if (held != tab.bytes_held() || store.size() != tab.blocks_held()) {
      std::printf("ERROR the table holds %zu bytes in %zu blocks, the store %zu in %zu\n", tab.bytes_held(),
                  tab.blocks_held(), held, store.size());
      return 1;
    }
    std::printf("bytes=%zu peak=%zu blocks=%zu freed=", tab.bytes_held(), peak, tab.blocks_held());
    for (size_t i = 0; i < freed.size(); i++) std::printf("%s%u", i ? "," : "", freed[i]);
    std::printf(" |");
    for (size_t s = 0; s < nslots + 2; s++) {  // two past the table: never any members
      const View v = tab.get(s);
      if (v.block == kNoBlock) {
        if (tab.count(s) != 0) return 1;
        continue;
      }
      const std::vector<uint32_t> &idx = *store.at(v.block).idx;  // read through the view, as a kernel would
      std::printf(" %zu:%u:", s, v.len);
      for (uint32_t k = 0; k < v.len; k++) std::printf("%s%u", k ? "," : "", idx.at(v.off + k));
    }
    std::printf("\n");
  }
  // everything still held is released by a final clear
  tab.drop_from(0);
  for (uint32_t b : tab.take_dead()) {
    delete store.at(b).idx;
    store.erase(b);
  }
  if (!store.empty() || tab.bytes_held() != 0) {
    std::printf("ERROR %zu blocks leaked\n", store.size());
    return 1;
  }
  std::printf("members: OK\n");
  return 0;
}
