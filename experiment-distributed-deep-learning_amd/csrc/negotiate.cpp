// negotiate.cpp — see negotiate.h.
#include "negotiate.h"

#include <algorithm>
#include <iterator>

#include "engine.h"

namespace ddl {

const char *request_type_name(int type) {
    switch (type) {
        case kReqAllreduce: return "Allreduce";  // TensorAllreduceRequest.cc:10
        case kReqBroadcast: return "Broadcast";  // TensorBroadcastRequest.cc:10
        case kReqAllgather: return "Allgather";  // TensorAllgatherRequest.cc:10
        default: return "Unknown";
    }
}

int type_order(int type) {  // rank of the type name in byte order
    switch (type) {
        case kReqAllgather: return 0;
        case kReqAllreduce: return 1;
        case kReqBroadcast: return 2;
        default: return 3;
    }
}

namespace {
const int kTypeByOrder[3] = {kReqAllgather, kReqAllreduce, kReqBroadcast};
}

std::string wire_id(const ReqId &id) {
    DDL_REQUIRE(id.order >= 0 && id.order < 3, DDL_STATUS_ERROR_UNKNOWN, "bad request id");
    return std::string(request_type_name(kTypeByOrder[id.order])) + "::" + id.key;
}

ReqId parse_wire_id(const std::string &s) {
    const size_t sep = s.find("::");
    DDL_REQUIRE(sep != std::string::npos, DDL_STATUS_COMM_ERROR, "token: malformed request id '" << s << "'");
    const std::string name = s.substr(0, sep);
    for (int o = 0; o < 3; ++o)
        if (name == request_type_name(kTypeByOrder[o])) return ReqId{o, s.substr(sep + 2)};
    fail(DDL_STATUS_COMM_ERROR, "token: unknown request type '" + name + "'");
}

std::shared_ptr<ControlChannel> &standalone_control() {
    static auto *ch = new std::shared_ptr<ControlChannel>(std::make_shared<ControlChannel>());
    return *ch;
}

namespace {
// Rank 0's view of one round: the agreed set is the proposal's entries that every member kept.
// String rounds: each answer is a subsequence of the proposal (members walk it in order).
// Cached rounds: index sets.
Agreed decide(bool cached, const std::vector<uint32_t> &idx, const std::vector<std::string> &strs,
              const std::vector<Token> &answers, ControlChannel &ch) {
    Agreed a;
    a.cached = cached;
    if (cached) {
        std::vector<uint32_t> agreed(idx);
        std::sort(agreed.begin(), agreed.end());
        for (const Token &t : answers) {
            std::vector<uint32_t> theirs = ch.cache.decode(t.msg);
            std::sort(theirs.begin(), theirs.end());
            std::vector<uint32_t> both;
            std::set_intersection(agreed.begin(), agreed.end(), theirs.begin(), theirs.end(), std::back_inserter(both));
            agreed.swap(both);
        }
        a.idx = std::move(agreed);
        return a;
    }
    std::vector<int> kept(strs.size(), 0);
    for (const Token &t : answers) {
        size_t j = 0;
        for (const std::string &k : decode_keys(t.msg)) {
            while (j < strs.size() && strs[j] != k) ++j;
            DDL_REQUIRE(j < strs.size(), DDL_STATUS_COMM_ERROR, "token protocol: answer '" << k << "' not proposed");
            ++kept[j++];
        }
    }
    for (size_t j = 0; j < strs.size(); ++j)
        if (kept[j] == (int)answers.size()) a.wire.push_back(strs[j]);
    return a;
}
}  // namespace

Agreed negotiate_root(ControlChannel &ch, bool cached, const std::vector<uint32_t> &idx,
                      const std::vector<std::string> &strs, int request_type,
                      const std::function<long long()> &snapshot) {
    const uint64_t cfg = config().shared_hash();
    Token t;
    t.type = cached ? TOKEN_SYNC_CACHED : TOKEN_SYNC;
    t.request = (uint8_t)request_type;
    t.cfg = cfg;
    t.msg = cached ? ch.cache.encode(idx) : encode_keys(strs);
    ch.send(t);  // the proposal to every member
    std::vector<Token> answers(ch.size() - 1);
    bool cfg_ok = true;
    long long release = -1;
    std::vector<uint64_t> hashes(ch.size(), cfg);
    for (int r = 1; r < ch.size(); ++r) {
        ch.recv_from(r, answers[r - 1], -1);
        DDL_REQUIRE(answers[r - 1].type == t.type, DDL_STATUS_COMM_ERROR,
                    "token protocol: expected SYNC from rank " << r << ", got " << (int)answers[r - 1].type);
        hashes[r] = answers[r - 1].cfg;
        cfg_ok = cfg_ok && answers[r - 1].cfg == cfg;
        release = std::max<long long>(release, answers[r - 1].seq);
    }
    if (snapshot) release = std::max(release, snapshot());
    Agreed a = decide(cached, idx, strs, answers, ch);
    a.cfg_ok = cfg_ok;
    a.release = release;
    if (!cfg_ok) {
        try {
            check_config_agreement(0, hashes);
        } catch (const Error &e) {
            DDL_LOG(0, "keyed round refused: " << e.msg);
        }
    }
    Token c;
    c.type = cached ? TOKEN_COMMUNICATE_CACHED : TOKEN_COMMUNICATE;
    c.request = (uint8_t)request_type;
    c.cfg = cfg_ok ? cfg : kCfgMismatch;
    c.seq = release;
    c.msg = cached ? ch.cache.encode(a.idx) : encode_keys(a.wire);
    ch.send(c);  // the agreed set to every member
    if (cached) {
        ++ch.cached_rounds;
    } else {
        std::sort(a.wire.begin(), a.wire.end());
        ++ch.string_rounds;
    }
    return a;
}

Agreed negotiate_member(ControlChannel &ch, const Token &sync,
                        const std::function<std::vector<std::string>(const std::vector<std::string> &)> &by_string,
                        const std::function<std::vector<uint32_t>(const std::vector<uint32_t> &)> &by_index,
                        const std::function<long long()> &snapshot) {
    DDL_REQUIRE(sync.type == TOKEN_SYNC || sync.type == TOKEN_SYNC_CACHED, DDL_STATUS_COMM_ERROR,
                "token protocol: expected SYNC, got " << (int)sync.type);
    const bool cached = sync.type == TOKEN_SYNC_CACHED;
    Token s;
    s.type = sync.type;
    s.request = sync.request;
    s.msg = cached ? ch.cache.encode(by_index(ch.cache.decode(sync.msg))) : encode_keys(by_string(decode_keys(sync.msg)));
    // the config this rank runs the round under: read once its first proposed request is registered
    // (by_string / by_index wait for it), not when the proposal arrives
    s.cfg = config().shared_hash();
    s.seq = snapshot ? snapshot() : -1;
    ch.send(s);  // this rank's intersection with the proposal
    Token c;
    ch.recv(c, -1);
    DDL_REQUIRE(c.type == (cached ? TOKEN_COMMUNICATE_CACHED : TOKEN_COMMUNICATE), DDL_STATUS_COMM_ERROR,
                "token protocol: expected COMMUNICATE, got " << (int)c.type);
    Agreed a;
    a.cached = cached;
    a.cfg_ok = c.cfg != kCfgMismatch;
    a.release = c.seq;
    if (!a.cfg_ok)
        DDL_LOG(0, "keyed round refused: the ranks' shared tunables differ (this rank's config hash " << std::hex
                                                                                                   << s.cfg << std::dec << ")");
    if (cached) {
        a.idx = ch.cache.decode(c.msg);
        ++ch.cached_rounds;
    } else {
        a.wire = decode_keys(c.msg);
        std::sort(a.wire.begin(), a.wire.end());
        ++ch.string_rounds;
    }
    return a;
}

}  // namespace ddl
