// Paged-KV block manager (host side, N4 in SURVEY §2.2): the class, shared by the pybind11
// registration (block_manager.cpp) and the decode-slot batcher (slot_batcher.cpp).
//
// Prefix caching (opt-in at construction; off: a plain LIFO free list, one private table per
// sequence, exactly as before).  On:
//   * every block has a reference count: the number of tables naming it.  free_sequence decrements,
//     deepest block first; an unregistered block at zero returns to the free list, a registered one
//     goes to the tail of an LRU list of EVICTABLE blocks and keeps its contents (a chain thus loses
//     its leaves before its root);
//   * a FULL block may be registered under a chained key: the parent block's key and its own
//     block_size token ids.  The index is a hash map, but a match is confirmed on the stored parent
//     link (the parent's registration id, unique for the manager's lifetime) and the stored token
//     ids, never on the hash alone.  Registering a key that exists keeps the older block;
//   * acquire_prefix builds a new sequence's table from the longest registered chain of its tokens,
//     capped at (len - 1) / block_size blocks: the last token is always computed, and no sequence
//     ever appends into a shared block;
//   * allocation takes from the free list first, then evicts the LRU head (dropping its
//     registration).  num_free / can_fit count evictable blocks as free, so the capacity the slot
//     batcher's preemption logic sees is the same as without the cache.
#pragma once

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <unordered_map>
#include <vector>

namespace py = pybind11;

class BlockManager {
 public:
  BlockManager(int num_blocks, int block_size, bool prefix_caching = false)
      : num_blocks_(num_blocks), block_size_(block_size), caching_(prefix_caching) {
    if (num_blocks <= 0 || block_size <= 0) throw std::invalid_argument("num_blocks/block_size must be > 0");
    free_.reserve(num_blocks);
    for (int b = num_blocks - 1; b >= 0; --b) free_.push_back(b);
    if (caching_) {
      ref_.assign(num_blocks, 0);
      uid_.assign(num_blocks, 0);
      parent_uid_.assign(num_blocks, 0);
      key_.assign(num_blocks, 0);
      tokens_.assign((size_t)num_blocks * block_size, 0);
      // LRU list of evictable blocks, intrusive, with the sentinel num_blocks (head = next of it)
      prev_.assign(num_blocks + 1, -1);
      next_.assign(num_blocks + 1, -1);
      prev_[num_blocks] = next_[num_blocks] = num_blocks;
    }
  }

  int num_blocks() const { return num_blocks_; }
  int block_size() const { return block_size_; }
  bool prefix_caching() const { return caching_; }
  int num_free() const { return (int)free_.size() + num_evictable_; }
  int num_evictable() const { return num_evictable_; }
  int num_sequences() const { return (int)tables_.size(); }
  int blocks_for(int64_t tokens) const { return (int)((tokens + block_size_ - 1) / block_size_); }

  bool has_sequence(int64_t seq) const { return tables_.count(seq) != 0; }

  // Blocks a sequence still needs to hold `tokens` tokens in total.
  int extra_blocks_needed(int64_t seq, int64_t tokens) const {
    auto it = tables_.find(seq);
    const int have = it == tables_.end() ? 0 : (int)it->second.size();
    return std::max(0, blocks_for(tokens) - have);
  }

  bool can_fit(int64_t seq, int64_t tokens) const { return extra_blocks_needed(seq, tokens) <= num_free(); }

  // Direct table access for the native batcher (nullptr = unknown sequence).
  const std::vector<int32_t>* table(int64_t seq) const {
    auto it = tables_.find(seq);
    return it == tables_.end() ? nullptr : &it->second;
  }

  // Grow the sequence's table to hold `tokens` tokens. All-or-nothing.
  bool ensure_capacity(int64_t seq, int64_t tokens) {
    const int need = extra_blocks_needed(seq, tokens);
    if (need > num_free()) return false;
    auto& t = tables_[seq];
    for (int i = 0; i < need; ++i) t.push_back(take_block());
    return true;
  }

  // Grow every sequence i to lens[i] tokens, in order; returns the index of the first one that
  // does not fit (nothing allocated for it or after it), or -1 when all fit.  One call per
  // decode step instead of one per sequence.
  int64_t ensure_capacity_batch(py::array_t<int64_t, py::array::c_style> seqs,
                                py::array_t<int64_t, py::array::c_style> lens) {
    auto s = seqs.unchecked<1>();
    auto l = lens.unchecked<1>();
    if (s.shape(0) != l.shape(0)) throw std::invalid_argument("seqs/lens length mismatch");
    for (py::ssize_t i = 0; i < s.shape(0); ++i)
      if (!ensure_capacity(s(i), l(i))) return i;
    return -1;
  }

  void free_sequence(int64_t seq) {
    auto it = tables_.find(seq);
    if (it == tables_.end()) return;
    for (auto b = it->second.rbegin(); b != it->second.rend(); ++b) release_block(*b);
    tables_.erase(it);
  }

  std::vector<int32_t> block_table(int64_t seq) const {
    auto it = tables_.find(seq);
    if (it == tables_.end()) throw std::out_of_range("unknown sequence");
    return it->second;
  }

  // out[B, max_blocks] int32 (C-contiguous), rows padded with `pad`.
  void fill_block_tables(py::array_t<int64_t, py::array::c_style> seqs,
                         py::array_t<int32_t, py::array::c_style> out, int32_t pad) const {
    auto s = seqs.unchecked<1>();
    auto o = out.mutable_unchecked<2>();
    if (o.shape(0) < s.shape(0)) throw std::invalid_argument("block table buffer too small");
    const int mb = (int)o.shape(1);
    for (py::ssize_t i = 0; i < s.shape(0); ++i) {
      auto it = tables_.find(s(i));
      if (it == tables_.end()) throw std::out_of_range("unknown sequence in fill_block_tables");
      const auto& t = it->second;
      if ((int)t.size() > mb) throw std::invalid_argument("sequence has more blocks than max_blocks");
      int j = 0;
      for (; j < (int)t.size(); ++j) o(i, j) = t[j];
      for (; j < mb; ++j) o(i, j) = pad;
    }
  }

  // Slot ids for tokens [start[i], start[i]+count[i]) of each sequence, packed in order.
  int fill_slots(py::array_t<int64_t, py::array::c_style> seqs, py::array_t<int32_t, py::array::c_style> start,
                 py::array_t<int32_t, py::array::c_style> count, py::array_t<int32_t, py::array::c_style> out) const {
    auto s = seqs.unchecked<1>();
    auto st = start.unchecked<1>();
    auto ct = count.unchecked<1>();
    auto o = out.mutable_unchecked<1>();
    py::ssize_t k = 0;
    for (py::ssize_t i = 0; i < s.shape(0); ++i) {
      auto it = tables_.find(s(i));
      if (it == tables_.end()) throw std::out_of_range("unknown sequence in fill_slots");
      const auto& t = it->second;
      for (int p = st(i); p < st(i) + ct(i); ++p) {
        const int bi = p / block_size_;
        if (bi >= (int)t.size()) throw std::out_of_range("token position beyond allocated blocks");
        if (k >= o.shape(0)) throw std::invalid_argument("slot buffer too small");
        o(k++) = t[bi] * block_size_ + p % block_size_;
      }
    }
    return (int)k;
  }

  // ------------------------------------------------------------------ prefix cache
  using Tokens = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;

  // Chained keys of the first `nblocks` full blocks of `tokens` (all of them with nblocks < 0): what
  // the scheduler's pending index is keyed by.  The hash only; a match in the manager compares more.
  std::vector<uint64_t> prefix_keys(Tokens tokens, int nblocks) const {
    auto t = tokens.unchecked<1>();
    int n = (int)(t.shape(0) / block_size_);
    if (nblocks >= 0) n = std::min(n, nblocks);
    std::vector<uint64_t> keys;
    keys.reserve(std::max(0, n));
    uint64_t key = 0;
    for (int i = 0; i < n; ++i) {
      key = chain_key(key, t.data(0) + (size_t)i * block_size_);
      keys.push_back(key);
    }
    return keys;
  }

  // Registered blocks a new sequence with these tokens would share (no side effect, no counters).
  int match_prefix(Tokens tokens) const {
    if (!caching_) return 0;
    auto t = tokens.unchecked<1>();
    std::vector<int32_t> chain;
    match(t.data(0), (int64_t)t.shape(0), chain);
    return (int)chain.size();
  }

  // Build the table of the NEW sequence `seq` from the longest registered prefix of `tokens`, at most
  // (len - 1) / block_size blocks; returns the number of cached tokens (0 with the cache off).
  // count_query: add the tokens to the queried-tokens counter (false when the caller asks again for a
  // sequence whose earlier query found nothing and that could not be admitted then).
  int64_t acquire_prefix(int64_t seq, Tokens tokens, bool count_query = true) {
    if (!caching_) return 0;
    if (seq < 0) throw std::invalid_argument("acquire_prefix: the scratch sequence shares nothing");
    if (tables_.count(seq)) throw std::invalid_argument("acquire_prefix: the sequence already has a table");
    auto t = tokens.unchecked<1>();
    std::vector<int32_t> chain;
    match(t.data(0), (int64_t)t.shape(0), chain);
    if (count_query) query_tokens_ += (int64_t)t.shape(0);
    if (chain.empty()) return 0;
    for (int32_t b : chain) {
      if (ref_[b]++ == 0) lru_remove(b);
    }
    const int64_t n = (int64_t)chain.size() * block_size_;
    hit_tokens_ += n;
    tables_[seq] = std::move(chain);
    return n;
  }

  // Register the full blocks of `seq` that hold tokens[0, num_tokens) (their K/V must be in the
  // cache: the step that computed them has completed).  Returns how many blocks became registered.
  int register_prefix(int64_t seq, Tokens tokens, int64_t num_tokens) {
    if (!caching_ || seq < 0) return 0;
    auto it = tables_.find(seq);
    if (it == tables_.end()) return 0;
    auto t = tokens.unchecked<1>();
    const auto& tab = it->second;
    const int n = (int)std::min<int64_t>({num_tokens / block_size_, t.shape(0) / block_size_, (int64_t)tab.size()});
    uint64_t key = 0, parent = 0;
    int added = 0;
    for (int i = 0; i < n; ++i) {
      const int32_t* tk = t.data(0) + (size_t)i * block_size_;
      key = chain_key(key, tk);
      const int32_t b = tab[i];
      if (b == 0) break;                                   // the scratch block is never registered
      if (uid_[b] != 0) {
        // already registered (it was matched, or registered by an earlier chunk): the same tokens, or
        // a table names a block with other contents.  Its parent link is stale when the older block
        // it was chained behind has been evicted and this sequence's private copy took its place:
        // the chain is the same content, so the link moves over (unless that key exists by now)
        if (!same_tokens(b, tk)) throw std::logic_error("registered block with other tokens in a table");
        if (parent_uid_[b] != parent) {
          const int32_t other = find(key, parent, tk);
          if (other >= 0) {
            parent = uid_[other];
            continue;
          }
          parent_uid_[b] = parent;
        }
        parent = uid_[b];
        continue;
      }
      const int32_t older = find(key, parent, tk);
      if (older >= 0) {                                    // duplicate: keep the older, b stays private
        parent = uid_[older];
        continue;
      }
      uid_[b] = ++next_uid_;
      parent_uid_[b] = parent;
      key_[b] = key & hash_mask_;
      std::memcpy(&tokens_[(size_t)b * block_size_], tk, sizeof(int32_t) * block_size_);
      index_.emplace(key_[b], b);
      ++num_registered_;
      ++added;
      parent = uid_[b];
    }
    return added;
  }

  int ref_count(int32_t b) const { return caching_ ? ref_.at(b) : -1; }
  bool is_registered(int32_t b) const { return caching_ && uid_.at(b) != 0; }
  int num_registered() const { return num_registered_; }

  // Evictable blocks, next to be evicted first.
  std::vector<int32_t> evictable_blocks() const {
    std::vector<int32_t> out;
    if (caching_)
      for (int b = next_[num_blocks_]; b != num_blocks_; b = next_[b]) out.push_back(b);
    return out;
  }

  std::vector<int32_t> free_blocks() const { return free_; }

  // (queried tokens, hit tokens, evictions, registered blocks)
  py::tuple prefix_stats() const { return py::make_tuple(query_tokens_, hit_tokens_, evictions_, num_registered_); }

  // Test hook: AND every key with `mask` before it enters or is looked up in the index (0: every
  // block collides with every other, so only the parent link and the token ids tell them apart).
  void set_hash_mask(uint64_t mask) {
    if (num_registered_) throw std::logic_error("set_hash_mask on a manager with registered blocks");
    hash_mask_ = mask;
  }

 private:
  uint64_t chain_key(uint64_t parent_key, const int32_t* tk) const {
    uint64_t h = parent_key ^ 0x9e3779b97f4a7c15ull;
    for (int i = 0; i < block_size_; ++i) {               // splitmix64 finaliser per token
      h += (uint64_t)(uint32_t)tk[i] + 0x9e3779b97f4a7c15ull;
      h = (h ^ (h >> 30)) * 0xbf58476d1ce4e5b9ull;
      h = (h ^ (h >> 27)) * 0x94d049bb133111ebull;
      h ^= h >> 31;
    }
    return h;
  }

  bool same_tokens(int32_t b, const int32_t* tk) const {
    return std::memcmp(&tokens_[(size_t)b * block_size_], tk, sizeof(int32_t) * block_size_) == 0;
  }

  // The registered block with this key, parent registration and token ids, or -1.
  int32_t find(uint64_t key, uint64_t parent, const int32_t* tk) const {
    auto range = index_.equal_range(key & hash_mask_);
    for (auto it = range.first; it != range.second; ++it) {
      const int32_t b = it->second;
      if (parent_uid_[b] == parent && same_tokens(b, tk)) return b;
    }
    return -1;
  }

  void match(const int32_t* tk, int64_t len, std::vector<int32_t>& chain) const {
    const int64_t cap = len > 0 ? (len - 1) / block_size_ : 0;
    uint64_t key = 0, parent = 0;
    for (int64_t i = 0; i < cap; ++i) {
      key = chain_key(key, tk + i * block_size_);
      const int32_t b = find(key, parent, tk + i * block_size_);
      if (b < 0) break;
      chain.push_back(b);
      parent = uid_[b];
    }
  }

  void lru_remove(int32_t b) {
    next_[prev_[b]] = next_[b];
    prev_[next_[b]] = prev_[b];
    prev_[b] = next_[b] = -1;
    --num_evictable_;
  }

  void lru_push_tail(int32_t b) {
    const int s = num_blocks_;
    prev_[b] = prev_[s];
    next_[b] = s;
    next_[prev_[s]] = b;
    prev_[s] = b;
    ++num_evictable_;
  }

  void unregister(int32_t b) {
    auto range = index_.equal_range(key_[b]);
    for (auto it = range.first; it != range.second; ++it)
      if (it->second == b) {
        index_.erase(it);
        break;
      }
    uid_[b] = 0;
    --num_registered_;
  }

  int32_t take_block() {
    int32_t b;
    if (!free_.empty()) {
      b = free_.back();
      free_.pop_back();
    } else {
      b = caching_ ? next_[num_blocks_] : num_blocks_;     // LRU head; the caller checked num_free()
      if (b == num_blocks_) throw std::logic_error("take_block with nothing free");
      lru_remove(b);
      unregister(b);
      ++evictions_;
    }
    if (caching_) ref_[b] = 1;
    return b;
  }

  void release_block(int32_t b) {
    if (!caching_) {
      free_.push_back(b);
      return;
    }
    if (--ref_[b] > 0) return;
    if (uid_[b] != 0) lru_push_tail(b);
    else free_.push_back(b);
  }

  int num_blocks_;
  int block_size_;
  bool caching_;
  std::vector<int32_t> free_;
  std::unordered_map<int64_t, std::vector<int32_t>> tables_;
  // prefix cache (sized only when caching_)
  std::vector<int32_t> ref_;
  std::vector<uint64_t> uid_;          // registration id, 0 = not registered
  std::vector<uint64_t> parent_uid_;   // registration id of the chain's previous block, 0 = first block
  std::vector<uint64_t> key_;          // masked chained key the block is indexed under
  std::vector<int32_t> tokens_;        // [num_blocks, block_size] token ids of registered blocks
  std::vector<int32_t> prev_, next_;
  std::unordered_multimap<uint64_t, int32_t> index_;
  uint64_t next_uid_ = 0;
  uint64_t hash_mask_ = ~0ull;
  int num_evictable_ = 0;
  int num_registered_ = 0;
  int64_t query_tokens_ = 0, hit_tokens_ = 0, evictions_ = 0;
};
