// Host-side validation of the caller's peer lists (av_set_peer_lists, rule R6) and their conversion
// to the device's 32-bit form. Plain C++17 with no HIP include, so a stand-alone program can run it
// under a host sanitizer. The listed draw (peer_lists.h) indexes the list by these offsets and the
// preference table by these ids with no further check: whatever passes here must be safe there.
#pragma once

#include <cstdint>
#include <vector>

namespace avk {

enum class PeerListError : int {
  Ok = 0,
  Null,        // peers == nullptr with a non-empty total
  FirstOffset, // offsets[0] != 0
  Decreasing,  // offsets[i + 1] < offsets[i]
  TooLong,     // the total is >= 2^31
  Range,       // a peer outside [0, n_nodes)
  Self,        // a node lists itself
  Order,       // a list is not strictly ascending (this also rejects duplicates)
};

inline const char* peer_list_error_text(PeerListError e) {
  switch (e) {
    case PeerListError::Ok: return "ok";
    case PeerListError::Null: return "null peer array";
    case PeerListError::FirstOffset: return "offsets[0] is not 0";
    case PeerListError::Decreasing: return "offsets decrease";
    case PeerListError::TooLong: return "2^31 list entries or more";
    case PeerListError::Range: return "a peer outside the network";
    case PeerListError::Self: return "a node lists itself";
    case PeerListError::Order: return "a list is not strictly ascending";
  }
  return "?";
}

// The lists of local nodes node_begin + i, i < local_nodes: peers[offsets[i] .. offsets[i + 1]). On
// Ok, off32 (local_nodes + 1 entries) and list32 hold them; on any error both are left as they were.
// *bad_node: the local index of the first offending list (or -1).
inline PeerListError check_peer_lists(int64_t n_nodes, int64_t node_begin, int64_t local_nodes, const int64_t* offsets,
                                      const int64_t* peers, std::vector<uint32_t>* off32,
                                      std::vector<uint32_t>* list32, int64_t* bad_node = nullptr) {
  if (bad_node) *bad_node = -1;
  if (offsets[0] != 0) return PeerListError::FirstOffset;
  for (int64_t i = 0; i < local_nodes; ++i) {
    if (bad_node) *bad_node = i;
    if (offsets[i + 1] < offsets[i]) return PeerListError::Decreasing;
    if (offsets[i + 1] >= (int64_t)1 << 31) return PeerListError::TooLong;
  }
  const int64_t total = offsets[local_nodes];
  if (total > 0 && !peers) return PeerListError::Null;
  for (int64_t i = 0; i < local_nodes; ++i) {
    if (bad_node) *bad_node = i;
    const int64_t self = node_begin + i;
    for (int64_t j = offsets[i]; j < offsets[i + 1]; ++j) {
      const int64_t q = peers[j];
      if (q < 0 || q >= n_nodes) return PeerListError::Range;
      if (q == self) return PeerListError::Self;
      if (j > offsets[i] && q <= peers[j - 1]) return PeerListError::Order;
    }
  }
  if (bad_node) *bad_node = -1;
  std::vector<uint32_t> o((size_t)local_nodes + 1), l((size_t)total);
  for (int64_t i = 0; i <= local_nodes; ++i) o[(size_t)i] = (uint32_t)offsets[i];
  for (int64_t j = 0; j < total; ++j) l[(size_t)j] = (uint32_t)peers[j];
  off32->swap(o);
  list32->swap(l);
  return PeerListError::Ok;
}

}  // namespace avk
