// teloscope_mi355x_ring.hpp — the chunks of one input dealt to several workers, for the read routes that use every context of a
// ReadTelomereFilter (include/teloscope_mi355x_io.hpp: fastqSubsetDevice, bamSubsetDevice).  Chunk k goes to worker k mod N, one
// host thread per worker (the arrangement ts_filter_reads_multi uses for the shards of a batch), and a chunk passes five steps:
//
//   take    the reader's turn, in chunk order: what the chunk's new bytes are (host work only);
//   stage   those bytes to the worker's device, beside the chunk they will join: any number of workers at once;
//   frame   the serial section, in chunk order: the unfinished record of chunk k - 1 goes in front, the staged bytes behind
//           it, and the records are framed, which says where chunk k's own unfinished record begins;
//   judge   the records judged and the passing ones gathered: any number of workers at once;
//   emit    the writer's turn, in chunk order.
//
// A turn waits for lower chunks only, so the lowest chunk always moves.  The first exception of the lowest chunk is what run()
// throws; no step of a higher chunk starts after it, and chunks below it finish as if nothing had happened — which is what a
// route on one worker does.  Nothing here knows about devices or formats: the steps are the caller's (Steps, below), and
// tests/cpp/read_ring_host.cpp runs the class over host buffers under the sanitizers.
#ifndef TELOSCOPE_MI355X_RING_HPP
#define TELOSCOPE_MI355X_RING_HPP

#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <exception>
#include <mutex>
#include <thread>
#include <vector>

namespace teloscope_mi355x {
namespace detail {

enum class RingTake { None, More, Last };       // there is no such chunk; a chunk, and more may follow; the input's last chunk

// Steps: void begin(size_t worker)                          once on the worker's thread, before its first chunk
//        RingTake take(size_t worker, uint64_t chunk)
//        void stage(size_t worker, uint64_t chunk)
//        bool frame(size_t worker, uint64_t chunk)          false: no chunk behind this one is framed (a record is not valid)
//        void judge(size_t worker, uint64_t chunk)
//        void emit(size_t worker, uint64_t chunk)
template <typename Steps>
class ChunkRing {
public:
    // chunks firstChunk, firstChunk + 1, ... ; chunk k is worker k mod `workers`'s
    ChunkRing(size_t workers, uint64_t firstChunk, Steps &steps) : n_(workers), first_(firstChunk), steps_(steps), waitMs_(workers, 0.0) {
        takeTurn_ = frameTurn_ = emitTurn_ = firstChunk;
    }

    void run() {
        std::vector<std::thread> threads;
        for (size_t w = 0; w < n_; ++w) threads.emplace_back([this, w] { work(w); });
        for (std::thread &t : threads) t.join();
        if (error_) std::rethrow_exception(error_);
    }

    // how long the worker waited for the chunk before its own to be framed: the serial section as the worker sees it
    double frameWaitMs(size_t worker) const { return waitMs_[worker]; }

private:
    static constexpr uint64_t kNoLimit = ~uint64_t(0);

    // waits until chunk k has the turn; false: chunk k does not run (the input ended or a lower chunk failed)
    bool await(uint64_t &turn, uint64_t k) {
        std::unique_lock<std::mutex> lock(m_);
        cv_.wait(lock, [&] { return turn == k || k >= limit_; });
        return k < limit_;
    }
    void pass(uint64_t &turn) {
        { std::lock_guard<std::mutex> lock(m_); ++turn; }
        cv_.notify_all();
    }
    void limit(uint64_t to) {
        { std::lock_guard<std::mutex> lock(m_); if (to < limit_) limit_ = to; }
        cv_.notify_all();
    }
    bool runs(uint64_t k) {
        std::lock_guard<std::mutex> lock(m_);
        return k < limit_;
    }

    void work(size_t w) {
        using Clock = std::chrono::steady_clock;
        uint64_t k = first_ + (w + n_ - first_ % n_) % n_;      // the worker's first chunk
        try {
            steps_.begin(w);
            for (; runs(k); k += n_) {
                if (!await(takeTurn_, k)) return;
                const RingTake took = steps_.take(w, k);
                if (took == RingTake::None) { limit(k); return; }
                if (took == RingTake::Last) limit(k + 1);
                pass(takeTurn_);
                steps_.stage(w, k);
                const Clock::time_point t0 = Clock::now();
                const bool framing = await(frameTurn_, k);
                waitMs_[w] += std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
                if (!framing) return;
                if (!steps_.frame(w, k)) limit(k + 1);
                pass(frameTurn_);
                steps_.judge(w, k);
                if (!await(emitTurn_, k)) return;
                steps_.emit(w, k);
                pass(emitTurn_);
            }
        } catch (...) {
            {
                std::lock_guard<std::mutex> lock(m_);
                if (!error_ || k < errorChunk_) { error_ = std::current_exception(); errorChunk_ = k; }
                if (k < limit_) limit_ = k;
            }
            cv_.notify_all();
        }
    }

    size_t n_;
    uint64_t first_;
    Steps &steps_;
    std::vector<double> waitMs_;
    std::mutex m_;
    std::condition_variable cv_;
    uint64_t takeTurn_ = 0, frameTurn_ = 0, emitTurn_ = 0, limit_ = kNoLimit;
    std::exception_ptr error_;
    uint64_t errorChunk_ = 0;
};

}  // namespace detail
}  // namespace teloscope_mi355x

#endif
