// readback_check.cpp -- the Newton loop's read-back layout, builders and decoders (csrc/readback.hpp) for
// tests/test_readback_host.py, which builds it with plain g++ (the header is host-only code) and feeds it one command per line
// on stdin.  Doubles travel as the 16 hex digits of their bit pattern, so NaN and Inf arrive and leave unchanged.
//   slots
//   plain NJOBS COUNT SLOT                      -> the FinishParams of finish_plain
//   trial_params HAS_F0 F0_COUNT COUNT SEQ      -> of finish_trial_params
//   dir_params COUNT SEQ                        -> of finish_direction_params
//   decode_trial STAMP b0 .. b15                -> value sumsq bad moved
//   decode_dir b0 .. b15                        -> sumsq bad gdotv pivot leaf
//   shard_trial R STAMP (b0 .. b15) x R         -> pack per rank, element-wise sum in rank order, unpack
//   shard_dir R (FAILED b0 .. b15) x R          -> the same for a direction; FAILED is the rank's status flag
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../multigridbarrier.jl_amd/csrc/readback.hpp"

using namespace mgbhip;

namespace {

constexpr uint64_t GUARD = 0x7ff8c0ffee123456ull;      // a NaN payload no test input uses

double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
uint64_t bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }

double read_double(std::istream& in) {
    std::string h;
    in >> h;
    return from_bits(strtoull(h.c_str(), nullptr, 16));
}
std::vector<double> read_block(std::istream& in) {
    std::vector<double> b((size_t)RB_SLOTS);         // exactly the block: a decoder that reads past it trips the sanitizer
    for (double& v : b) v = read_double(in);
    return b;
}

// pointers of a FinishParams are printed as offsets into these (or "null" / "other")
double g_partials[4096], g_f0[1], g_block[1], g_host[1];      // rows of partials: NJOBS * COUNT <= 4096
int32_t g_ints[1];

void print_params(const FinishParams& F) {
    printf("njobs %d", F.njobs);
    for (int k = 0; k < F.njobs; ++k) {
        const char* base = "partials";
        long off = (long)(F.job[k].src - g_partials);
        if (F.job[k].src == g_f0) { base = "f0"; off = 0; }
        printf(" job %s %ld %" PRId64 " %d", base, off, F.job[k].count, F.job[k].out);
    }
    printf(" out %s ints %s nints %d ints_out %d reset %d host %s host_lo %d host_n %d seq %.17g\n",
           F.out == g_block ? "block" : "other", F.ints == nullptr ? "null" : (F.ints == g_ints ? "ints" : "other"), F.nints,
           F.ints_out, F.reset, F.host == nullptr ? "null" : (F.host == g_host ? "host" : "other"), F.host_lo, F.host_n, F.seq);
}

// pack into the middle of a guarded array: exactly RB_SHARD doubles are written
template <class Pack>
std::vector<double> guarded_pack(Pack pack) {
    std::vector<double> buf((size_t)RB_SHARD + 2, from_bits(GUARD));
    pack(buf.data() + 1);
    int written = 0;
    for (int k = 0; k < RB_SHARD; ++k) written += bits(buf[(size_t)k + 1]) != GUARD;
    const bool guards = bits(buf.front()) == GUARD && bits(buf.back()) == GUARD;
    printf("packed %d guards %d ", written, guards ? 1 : 0);
    return std::vector<double>(buf.begin() + 1, buf.end() - 1);
}

void print_sums(const std::vector<double>& s) {
    printf("sums");
    for (double v : s) printf(" %016" PRIx64, bits(v));
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "slots") {
            printf("VALUE %d AUX %d SUMSQ %d BAD %d MOVED %d GDOTV %d PIVOT %d LEAF %d STAMP %d SLOTS %d SHARD %d\n", (int)RB_VALUE,
                   (int)RB_AUX, (int)RB_SUMSQ, (int)RB_BAD, (int)RB_MOVED, (int)RB_GDOTV, (int)RB_PIVOT, (int)RB_LEAF, (int)RB_STAMP,
                   (int)RB_SLOTS, RB_SHARD);
        } else if (cmd == "plain") {
            int njobs, slot; long count;
            in >> njobs >> count >> slot;
            print_params(finish_plain(g_partials, count, njobs, g_block, slot));
        } else if (cmd == "trial_params") {
            int has_f0; long f0_count, count; double seq;
            in >> has_f0 >> f0_count >> count >> seq;
            print_params(finish_trial_params(has_f0 ? g_f0 : nullptr, f0_count, g_partials, count, g_block, g_ints, g_host, seq));
        } else if (cmd == "dir_params") {
            long count; double seq;
            in >> count >> seq;
            print_params(finish_direction_params(g_partials, count, g_block, g_ints, g_host, seq));
        } else if (cmd == "decode_trial") {
            int32_t stamp;
            in >> stamp;
            const std::vector<double> b = read_block(in);
            const TrialReadback r = decode_trial(b.data(), stamp);
            printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d\n", bits(r.value), bits(r.sumsq), bits(r.bad), r.moved ? 1 : 0);
        } else if (cmd == "decode_dir") {
            const std::vector<double> b = read_block(in);
            const DirReadback r = decode_direction(b.data());
            printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d %d\n", bits(r.sumsq), bits(r.bad), bits(r.gdotv), r.pivot ? 1 : 0,
                   r.leaf ? 1 : 0);
        } else if (cmd == "shard_trial") {
            int R; int32_t stamp;
            in >> R >> stamp;
            std::vector<double> sum;
            for (int rank = 0; rank < R; ++rank) {
                const std::vector<double> b = read_block(in);
                const TrialReadback r = decode_trial(b.data(), stamp);
                const std::vector<double> s = guarded_pack([&](double* p) { pack_trial(r, p); });
                if (rank == 0) sum = s;
                else for (size_t k = 0; k < s.size(); ++k) sum[k] += s[k];
            }
            const TrialReadback r = unpack_trial(sum.data());
            print_sums(sum);
            printf(" record %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d\n", bits(r.value), bits(r.sumsq), bits(r.bad), r.moved ? 1 : 0);
        } else if (cmd == "shard_dir") {
            int R;
            in >> R;
            std::vector<double> sum;
            DirReadback last{};
            for (int rank = 0; rank < R; ++rank) {
                int failed;
                in >> failed;
                const std::vector<double> b = read_block(in);
                last = decode_direction(b.data());
                const std::vector<double> s = guarded_pack([&](double* p) { pack_direction(last, failed != 0, p); });
                if (rank == 0) sum = s;
                else for (size_t k = 0; k < s.size(); ++k) sum[k] += s[k];
            }
            const bool any_failed = unpack_direction(sum.data(), last);
            print_sums(sum);
            printf(" record %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " failed %d\n", bits(last.sumsq), bits(last.bad), bits(last.gdotv),
                   any_failed ? 1 : 0);
        } else {
            fprintf(stderr, "unknown command: %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
