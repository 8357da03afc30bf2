// Resident committee member lists, host bookkeeping (include/grandine_bls_gpu_bits.h).  Host-only
// and free of HIP so that tests/native/members_main.cpp runs it under ASan/UBSan against a model.
//
// Every gbls_committees_set_members call uploads its index lists as ONE block per engine device
// (they are uploaded for the sums anyway); a slot with members is an (offset, length) into a block.
// A block lives while a slot points into it.  A slot is rewritten every epoch with another size, so
// nothing is rewritten in place: the new call's block replaces the slot's view and the old block
// dies with its last slot.  Dead blocks are handed out once by take_dead(); the engine frees their
// device memory behind the kernels that may still read them (the registry's retire discipline:
// readers enqueue under the shared registry lock and mark Ctx::ev_reg, a writer holds the lock
// exclusively, so every reader of a block that dies in a write was enqueued before that write).
//
// Memory bound.  A block holds 4 bytes per index of its call.  A block is held whole while any of
// its slots is live, so the bytes held are at most the bytes of the calls that still own a slot.
// In a steady epoch rollover (halves A and B of the table rewritten alternately, each rewrite
// covering its whole half) a rewrite of A kills the previous block of A in the same call: two
// blocks are held between calls, and within a call (the new block is made before the old one
// dies) three -- below the bytes of three halves, whatever the committee sizes.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gbls {
namespace members {

constexpr uint32_t kNoBlock = 0xffffffffu;

struct View {
  uint32_t block = kNoBlock;  // kNoBlock: the slot keeps no members
  uint32_t off = 0, len = 0;  // indices [off, off + len) of the block
};

class Table {
 public:
  // a block of nidx indices, owned by no slot yet; close_block() after its slots are assigned
  uint32_t open_block(size_t nidx) {
    uint32_t id;
    if (!spare_.empty()) {
      id = spare_.back();
      spare_.pop_back();
    } else {
      id = (uint32_t)blocks_.size();
      blocks_.push_back(Block());
    }
    blocks_[id] = Block{0, nidx, true, ++serial_};
    bytes_ += nidx * 4;
    return id;
  }
  // slot views [off, off + len) of block; the slot's previous members are dropped
  void assign(size_t slot, uint32_t block, uint32_t off, uint32_t len) {
    if (slot >= slots_.size()) slots_.resize(slot + 1);
    drop(slot);
    slots_[slot] = View{block, off, len};
    blocks_[block].live++;
  }
  // the call that opened the block has assigned its slots: without any, the block is dead
  void close_block(uint32_t block) {
    blocks_[block].open = false;
    if (blocks_[block].live == 0) kill(block);
  }
  void drop(size_t slot) {
    if (slot >= slots_.size() || slots_[slot].block == kNoBlock) return;
    const uint32_t b = slots_[slot].block;
    slots_[slot] = View();
    if (--blocks_[b].live == 0 && !blocks_[b].open) kill(b);
  }
  // slots first.. lose their members (a truncation; first = 0: gbls_committees_clear, a registry rewrite)
  void drop_from(size_t first) {
    for (size_t s = first; s < slots_.size(); s++) drop(s);
    if (first < slots_.size()) slots_.resize(first);
  }
  // Drops the slot's view if it still points into the block that open_block() returned as `block`
  // with serial `serial` (a call dropping the slots whose status came back nonzero, after the lock
  // was released: a later call may have rewritten them meanwhile, and the id may have been reused).
  uint64_t serial(uint32_t block) const { return blocks_[block].serial; }
  void drop_if(size_t slot, uint32_t block, uint64_t serial) {
    if (slot < slots_.size() && slots_[slot].block == block && blocks_[block].serial == serial) drop(slot);
  }
  View get(size_t slot) const { return slot < slots_.size() ? slots_[slot] : View(); }
  size_t count(size_t slot) const { return get(slot).block == kNoBlock ? 0 : get(slot).len; }
  size_t bytes_held() const { return bytes_; }  // blocks not yet handed out by take_dead()
  size_t blocks_held() const { return blocks_.size() - spare_.size(); }
  // the blocks that died since the last call, each handed out once: the caller frees their device
  // memory; their ids are reused by later open_block()s
  std::vector<uint32_t> take_dead() {
    std::vector<uint32_t> out;
    out.swap(dead_);
    for (uint32_t b : out) {
      bytes_ -= blocks_[b].nidx * 4;
      blocks_[b] = Block();
      spare_.push_back(b);
    }
    return out;
  }

 private:
  struct Block {
    uint32_t live = 0;  // slots pointing into it
    size_t nidx = 0;
    bool open = false;
    uint64_t serial = 0;  // of the open_block() that made it
  };
  void kill(uint32_t b) { dead_.push_back(b); }
  std::vector<View> slots_;
  std::vector<Block> blocks_;
  std::vector<uint32_t> dead_, spare_;
  size_t bytes_ = 0;
  uint64_t serial_ = 0;
};

}  // namespace members
}  // namespace gbls
