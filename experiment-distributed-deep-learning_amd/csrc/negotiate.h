// negotiate.h — request ids on the wire and one negotiation round over the star (control.h): which
// keys every rank has registered. Used by the keyed handler (handler.h) and, without any handler,
// by ddl_control_negotiate (tools, CPU tests).
#pragma once

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "control.h"

namespace ddl {

// Request types, numbered as the reference's Token::RequestType (rtc/Token.h:23-29); the type
// name prefixes the key on the wire and in the pending map ("Allreduce::grad_0", as
// RingTokenCommunicateHandler.cc:140-146 builds its ready keys).
enum RequestType : int { kReqAllreduce = 1, kReqBroadcast = 2, kReqAllgather = 3 };
const char *request_type_name(int type);

// Request identity: (type, key), ordered as the reference's (typeName, key) pairs —
// "Allgather" < "Allreduce" < "Broadcast", then the key bytewise. On the wire it is the string
// "<TypeName>::<key>".
struct ReqId {
    int order;  // type_order(type)
    std::string key;
    bool operator<(const ReqId &o) const { return order != o.order ? order < o.order : key < o.key; }
};
int type_order(int type);
std::string wire_id(const ReqId &id);
ReqId parse_wire_id(const std::string &s);  // throws on an unknown type name

// The process's listening / standalone control channel: ddl_control_listen opens it,
// ddl_control_connect hands it to the world communicator (replacing it with a fresh one),
// ddl_control_connect_ranked keeps it for ddl_control_negotiate (tools, CPU tests).
std::shared_ptr<ControlChannel> &standalone_control();

// One negotiation round over the star (control.h).
//   root:   SYNC(proposal) to every member; every member's SYNC(intersection) back; the
//           proposal's ids every member kept go out as COMMUNICATE(agreed).
//   member: receives SYNC, intersects with what it holds (may block until the first proposed
//           id is registered), answers rank 0, then receives COMMUNICATE.
// A proposal made only of ids agreed in earlier rounds travels as indices into the channel's
// IdCache (TOKEN_*_CACHED) and is intersected by index; otherwise as "Type::key" strings.
// Every token also carries the sender's Config::shared_hash(): rank 0 compares the members'
// with its own and the COMMUNICATE says whether they all agree (cfg_ok); a round whose ranks
// disagree takes its agreed requests out on every rank and fails them with
// DDL_STATUS_CONFIG_MISMATCH instead of running them. `snapshot` (optional) freezes the rank's
// user collectives and returns how many it has issued (Communicator::round_freeze): members
// call it right before answering, rank 0 once every answer is in; the COMMUNICATE carries the
// maximum (release: the round goes after that many user collectives on every rank, -1 without
// snapshots).
struct Agreed {
    bool cached = false;
    std::vector<uint32_t> idx;      // cached round: indices into ch.cache
    std::vector<std::string> wire;  // string round: ids, sorted (their (type, key) order)
    bool cfg_ok = true;
    long long release = -1;
};
Agreed negotiate_root(ControlChannel &ch, bool cached, const std::vector<uint32_t> &idx,
                      const std::vector<std::string> &strs, int request_type = kReqAllreduce,
                      const std::function<long long()> &snapshot = nullptr);
Agreed negotiate_member(ControlChannel &ch, const Token &sync,
                        const std::function<std::vector<std::string>(const std::vector<std::string> &)> &by_string,
                        const std::function<std::vector<uint32_t>(const std::vector<uint32_t> &)> &by_index,
                        const std::function<long long()> &snapshot = nullptr);

}  // namespace ddl
