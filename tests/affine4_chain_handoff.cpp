// Stand-alone check of csrc/affine4_chain_value.hpp, the hand-off of one boundary value of the chained double-affine route as two
// 8-byte halves (tests/test_affine4_chain_handoff.py builds it under ThreadSanitizer and runs it).  One producer thread writes
// {M, I1, I2} of every column as two relaxed std::atomic<uint64_t> stores into a row preset to all-ones, lo first, hi first or in
// turns; one consumer thread, running at the same time, spins on delivered() with relaxed loads, as the kernel does.  Every column the
// consumer accepts must be the triple the producer wrote for it, the largest values (M = 2^30, I = 2^30 + 2000) and I2 = 0 among them,
// and a column with one half written must not be accepted.  Exit status 0 and "ok <columns> <rounds> <halves seen>" when all held, else
// the first violation on stderr and status 1.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <thread>

#include "affine4_chain_value.hpp"

using namespace pa::affine4_chain;

namespace {

constexpr int kCols = 6000;

struct Triple {
    uint32_t M, I1, I2;
};

// What the producer writes for column c in round r: the corners of the value range in turn, else values spread over it.
Triple triple_of(int c, int r) {
    switch (c % 8) {
        case 0: return Triple{kInf, kLayerMax, kLayerMax};
        case 1: return Triple{kInf, kLayerMax, 0};
        case 2: return Triple{0, 0, 0};
        case 3: return Triple{kInf, kInf, kInf};  // a column past |a|, as the kernel pads it
        default: {
            const uint64_t x = (uint64_t)(c + 1) * 2654435761u + (uint64_t)r * 40503u;
            return Triple{(uint32_t)(x % (kInf + 1ull)), (uint32_t)((x >> 7) % (kLayerMax + 1ull)), (uint32_t)((x >> 13) % (kLayerMax + 1ull))};
        }
    }
}

enum Order { kLoFirst, kHiFirst, kInTurns };

int fails = 0;
std::atomic<long> halves_seen{0};

void produce(std::atomic<uint64_t>* row, int r, Order order) {
    for (int c = 0; c < kCols; ++c) {
        const Triple t = triple_of(c, r);
        const Halves h = pack(t.M, t.I1, t.I2);
        const bool lo_first = order == kLoFirst || (order == kInTurns && c % 2 == 0);
        std::atomic<uint64_t>& first = row[2 * c + (lo_first ? 0 : 1)];
        std::atomic<uint64_t>& second = row[2 * c + (lo_first ? 1 : 0)];
        first.store(lo_first ? h.lo : h.hi, std::memory_order_relaxed);
        if (c % 16 == 5) std::this_thread::yield();  // leave the column half-written for a while
        second.store(lo_first ? h.hi : h.lo, std::memory_order_relaxed);
    }
}

void consume(const std::atomic<uint64_t>* row, int r) {
    for (int c = 0; c < kCols; ++c) {
        uint64_t lo, hi;
        for (;;) {
            lo = row[2 * c].load(std::memory_order_relaxed);
            hi = row[2 * c + 1].load(std::memory_order_relaxed);
            if (delivered(lo, hi)) break;
            if ((lo == kEmpty) != (hi == kEmpty)) halves_seen.fetch_add(1, std::memory_order_relaxed);  // one half there: not accepted
        }
        const Triple t = triple_of(c, r);
        if (m_of(lo) != t.M || i1_of(lo) != t.I1 || i2_of(hi) != t.I2 || (hi >> 32) != 0) {
            if (fails++ == 0)
                std::fprintf(stderr, "round %d column %d: accepted {%u, %u, %u | %u}, written {%u, %u, %u}\n", r, c, m_of(lo), i1_of(lo), i2_of(hi),
                             (uint32_t)(hi >> 32), t.M, t.I1, t.I2);
        }
    }
}

}  // namespace

int main() {
    // one thread: a column is accepted only with both halves, whichever comes first
    for (int c = 0; c < 8; ++c) {
        const Triple t = triple_of(c, 0);
        const Halves h = pack(t.M, t.I1, t.I2);
        if (delivered(kEmpty, kEmpty) || delivered(h.lo, kEmpty) || delivered(kEmpty, h.hi) || !delivered(h.lo, h.hi) || h.lo == kEmpty || h.hi == kEmpty) {
            std::fprintf(stderr, "delivered() is wrong for {%u, %u, %u}\n", t.M, t.I1, t.I2);
            return 1;
        }
    }
    const Order orders[] = {kLoFirst, kHiFirst, kInTurns, kInTurns};
    int rounds = 0;
    for (const Order order : orders) {
        std::unique_ptr<std::atomic<uint64_t>[]> row(new std::atomic<uint64_t>[2 * kCols]);
        for (int k = 0; k < 2 * kCols; ++k) row[k].store(kEmpty, std::memory_order_relaxed);  // the host's 0xFF fill
        const int r = rounds;
        // the last round starts the reader first, so that it is polling while the first columns arrive
        std::thread reader, writer;
        if (r == 3) {
            reader = std::thread(consume, row.get(), r);
            std::this_thread::yield();
            writer = std::thread(produce, row.get(), r, order);
        } else {
            writer = std::thread(produce, row.get(), r, order);
            reader = std::thread(consume, row.get(), r);
        }
        writer.join();
        reader.join();
        ++rounds;
    }
    if (fails) {
        std::fprintf(stderr, "%d columns differ\n", fails);
        return 1;
    }
    std::printf("ok %d %d %ld\n", kCols, rounds, halves_seen.load());
    return 0;
}
