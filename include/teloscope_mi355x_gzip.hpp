// teloscope_mi355x_gzip.hpp — the host's share of reading plain gzip for the device routes (detail::ChunkFeed's Gzip source in
// teloscope_mi355x_io.hpp): member headers and trailers (RFC 1952), and zlib as the judge of everything the device did not
// verify.  The device decodes windows of a member's deflate stream (include/teloscan.h: ts_gzip_decode) and says at which bit
// its verified chain of blocks ended and why; wherever that is short of the window's end, a raw inflate primed at exactly that
// bit, with the last 32 KiB as its dictionary, runs to the first block boundary past the window's edge (past the one block a
// span overflowed on or could not decode, where that is why the chain ended), and the device goes on from there.  What zlib says there is what the reader says: a data error or a failed trailer check is GzipError (gzread's
// -1), a truncated file delivers what zlib could still produce and ends quietly, further members follow, and bytes behind a
// member that are no gzip header end the input.  Nothing here needs a device: GzipDevice is an interface, and the host tests
// drive the reader with a stand-in (tests/cpp/gzip_feed_host.cpp).
#ifndef TELOSCOPE_MI355X_GZIP_HPP
#define TELOSCOPE_MI355X_GZIP_HPP

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include <zlib.h>

namespace teloscope_mi355x {
namespace detail {

struct GzipError : std::runtime_error { using std::runtime_error::runtime_error; };

// The gzip member header at p: its length; 0: p does not begin with the gzip magic; `truncated`: the input ends inside it.
// Throws GzipError for what zlib calls a data error there (unknown method, reserved flags, a header CRC that does not match).
inline size_t gzipHeaderLength(const unsigned char *p, size_t n, bool &truncated) {
    truncated = false;
    if (n < 2) { truncated = n == 1 && p[0] == 0x1f; return 0; }
    if (p[0] != 0x1f || p[1] != 0x8b) return 0;
    if (n < 10) { truncated = true; return 0; }
    if (p[2] != 8) throw GzipError("unknown compression method");
    const unsigned flags = p[3];
    if (flags & 0xe0) throw GzipError("unknown header flags set");
    size_t at = 10;
    if (flags & 4) {                                            // FEXTRA
        if (n - at < 2) { truncated = true; return 0; }
        const size_t xlen = p[at] | (static_cast<size_t>(p[at + 1]) << 8);
        at += 2;
        if (n - at < xlen) { truncated = true; return 0; }
        at += xlen;
    }
    for (unsigned bit : {8u, 16u})                              // FNAME, FCOMMENT: zero-terminated
        if (flags & bit) {
            const void *z = std::memchr(p + at, 0, n - at);
            if (!z) { truncated = true; return 0; }
            at = static_cast<size_t>(static_cast<const unsigned char *>(z) - p) + 1;
        }
    if (flags & 2) {                                            // FHCRC: the low 16 bits of the header's CRC32
        if (n - at < 2) { truncated = true; return 0; }
        const unsigned want = p[at] | (static_cast<unsigned>(p[at + 1]) << 8);
        if ((crc32(crc32(0L, Z_NULL, 0), p, static_cast<uInt>(at)) & 0xffffu) != want) throw GzipError("header crc mismatch");
        at += 2;
    }
    return at;
}

// what a device decode of one window answers (ts_gzip_result's fields)
struct GzipWindowResult { uint64_t endBit = 0, plainBytes = 0; uint32_t crc = 0; int status = 0; };
enum { kGzipWindowEnd = 0, kGzipFinalBlock = 1, kGzipNoCandidate = 2, kGzipSpanOverflow = 3, kGzipBadDeflate = 4 };
enum { kGzipHistoryEmpty = 0, kGzipHistoryKept = 1, kGzipHistoryGiven = 2 };

struct GzipDevice {
    virtual ~GzipDevice() = default;
    // window[0, n) from startBit (< 8) on; history as ts_gzip_decode takes it.  The bytes it produces stay with the device until
    // the next decode: the reader's caller fetches them when the reader hands out an OnDevice piece.
    virtual GzipWindowResult decode(const unsigned char *window, size_t n, unsigned startBit, int historyMode,
                                    const unsigned char *history, size_t historyLen) = 0;
    // the last <= 32 KiB in front of the last decode's end bit
    virtual void history(std::vector<unsigned char> &out) = 0;
    // a stretch of the input went to zlib (for the statistics)
    virtual void noteFallback() {}
};

// One input of gzip members -> pieces of plain bytes, in order.
class GzipReader {
public:
    enum Kind { None, OnDevice, OnHost };
    struct Tuning { size_t windowBytes = size_t(8) << 20, minBytes = size_t(1) << 20, hostPiece = size_t(1) << 20; };

    // data[at, size) begins with a gzip member (the caller has seen the magic); device may be null: zlib reads everything
    GzipReader(const unsigned char *data, size_t size, size_t at, GzipDevice *device, Tuning tuning)
        : data_(data), size_(size), at_(at), dev_(device), tune_(tuning) {
        tune_.windowBytes = std::max<size_t>(tune_.windowBytes, 1024);
        tune_.hostPiece = std::max<size_t>(tune_.hostPiece, 1);
    }
    GzipReader(const GzipReader &) = delete;
    GzipReader &operator=(const GzipReader &) = delete;
    ~GzipReader() { endZlib(); }

    uint64_t bytesLeft() const { return size_ - std::min(size_, at_); }     // compressed bytes not yet behind the reader
    uint64_t zlibBytes() const { return zlibBytes_; }                       // plain bytes zlib produced so far

    // The next piece: OnDevice — len bytes the device holds from its last decode; OnHost — host[0, len), valid until the next
    // call; None — the input is at its end.  Throws GzipError where gzread answers -1.
    Kind next(uint64_t &len, const char *&host) {
        len = 0; host = nullptr;
        for (;;) {
            switch (state_) {
            case Header: {
                bool truncated = false;
                const size_t h = at_ < size_ ? gzipHeaderLength(data_ + at_, size_ - at_, truncated) : 0;
                if (h == 0) { state_ = End; break; }            // the end, a cut header, or trailing bytes that are no member
                bit_ = 8 * static_cast<uint64_t>(at_ + h);
                crc_ = static_cast<uint32_t>(crc32(0L, Z_NULL, 0)); isize_ = 0;
                hist_.clear(); histMode_ = kGzipHistoryEmpty;
                edge_ = ~uint64_t(0);
                state_ = dev_ && size_ - at_ >= tune_.minBytes ? Device : Zlib;
                if (dev_ && state_ == Zlib) dev_->noteFallback();
                break;
            }
            case Device: {
                const size_t byte0 = static_cast<size_t>(bit_ / 8), n = std::min(tune_.windowBytes, size_ - byte0);
                if (n == 0) { state_ = End; break; }
                const GzipWindowResult r = dev_->decode(data_ + byte0, n, static_cast<unsigned>(bit_ & 7), histMode_, hist_.data(), hist_.size());
                if (r.endBit < (bit_ & 7) || r.endBit > 8 * static_cast<uint64_t>(n)) throw std::logic_error("gzip device: end bit outside the window");
                const uint64_t end = 8 * static_cast<uint64_t>(byte0) + r.endBit;
                const bool progress = end > bit_;
                bit_ = end;
                crc_ = static_cast<uint32_t>(crc32_combine(crc_, r.crc, static_cast<z_off_t>(r.plainBytes)));
                isize_ += r.plainBytes;
                if (r.status == kGzipFinalBlock) { at_ = static_cast<size_t>((bit_ + 7) / 8); state_ = Trailer; }
                else if (r.status == kGzipWindowEnd && progress && byte0 + n < size_) histMode_ = kGzipHistoryKept;
                else {                                          // zlib takes over at this bit, up to the first boundary past the window
                    dev_->history(hist_);
                    dev_->noteFallback();
                    // (a span that overflowed or met bad bits: zlib reads that one block and the device resumes behind it)
                    if (r.status == kGzipSpanOverflow || r.status == kGzipBadDeflate) edge_ = bit_ + 1;
                    else edge_ = byte0 + n < size_ ? 8 * static_cast<uint64_t>(byte0 + n) : ~uint64_t(0);
                    state_ = Zlib;
                }
                if (r.plainBytes) { len = r.plainBytes; return OnDevice; }
                break;
            }
            case Zlib: {
                if (!zOn_) beginZlib();
                if (out_.size() < tune_.hostPiece) out_.resize(tune_.hostPiece);
                z_.next_out = reinterpret_cast<Bytef *>(out_.data());
                z_.avail_out = static_cast<uInt>(std::min<size_t>(out_.size(), 1u << 30));
                const uInt room = z_.avail_out;
                State then = Zlib;
                while (z_.avail_out > 0) {
                    if (z_.avail_in == 0 && zNext_ < size_) {
                        z_.next_in = const_cast<Bytef *>(data_ + zNext_);
                        z_.avail_in = static_cast<uInt>(std::min<size_t>(size_ - zNext_, 1u << 30));
                        zNext_ += z_.avail_in;
                    }
                    const uInt inBefore = z_.avail_in, outBefore = z_.avail_out;
                    const int rc = inflate(&z_, Z_BLOCK);
                    const uint64_t pos = 8 * static_cast<uint64_t>(zNext_ - z_.avail_in) - static_cast<uint64_t>(z_.data_type & 63);
                    if (rc == Z_STREAM_END) { at_ = zNext_ - z_.avail_in; then = Trailer; break; }
                    if (rc != Z_OK && rc != Z_BUF_ERROR) { endZlib(); throw GzipError(rc == Z_MEM_ERROR ? "out of memory" : "invalid deflate data"); }
                    if ((z_.data_type & 128) && !(z_.data_type & 64) && pos >= edge_) { bit_ = pos; then = Device; break; }
                    if (z_.avail_in == inBefore && z_.avail_out == outBefore && z_.avail_in == 0 && zNext_ >= size_) { then = End; break; }   // cut short
                }
                const size_t made = room - z_.avail_out;
                crc_ = static_cast<uint32_t>(crc32(crc_, reinterpret_cast<const Bytef *>(out_.data()), static_cast<uInt>(made)));
                isize_ += made; zlibBytes_ += made;
                if (then == Device) {                           // the device goes on with zlib's last 32 KiB in front of it
                    hist_.resize(32768);
                    uInt got = 0;
                    if (inflateGetDictionary(&z_, hist_.data(), &got) != Z_OK) { endZlib(); throw GzipError("zlib keeps no window"); }
                    hist_.resize(got);
                    histMode_ = kGzipHistoryGiven;
                }
                if (then != Zlib) endZlib();
                state_ = then;
                if (made) { len = made; host = out_.data(); return OnHost; }
                break;
            }
            case Trailer: {
                if (size_ - std::min(size_, at_) < 8) { state_ = End; break; }      // cut inside the trailer: zlib ends quietly
                const unsigned char *t = data_ + at_;
                auto le32 = [](const unsigned char *p) { return static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8) | (static_cast<uint32_t>(p[2]) << 16) | (static_cast<uint32_t>(p[3]) << 24); };
                if (le32(t) != crc_) throw GzipError("incorrect data check");
                if (le32(t + 4) != static_cast<uint32_t>(isize_)) throw GzipError("incorrect length check");
                at_ += 8;
                state_ = Header;
                break;
            }
            case End:
                return None;
            }
        }
    }

private:
    enum State { Header, Device, Zlib, Trailer, End };

    // a raw inflate that continues at bit_ with hist_ as the 32 KiB in front of it
    void beginZlib() {
        std::memset(&z_, 0, sizeof z_);
        if (inflateInit2(&z_, -15) != Z_OK) throw GzipError("out of memory");
        zOn_ = true;
        zNext_ = static_cast<size_t>(bit_ / 8);
        const unsigned skip = static_cast<unsigned>(bit_ & 7);
        if (skip && zNext_ < size_) { inflatePrime(&z_, static_cast<int>(8 - skip), data_[zNext_] >> skip); ++zNext_; }
        if (!hist_.empty()) inflateSetDictionary(&z_, hist_.data(), static_cast<uInt>(hist_.size()));
        z_.avail_in = 0;
    }
    void endZlib() { if (zOn_) { inflateEnd(&z_); zOn_ = false; } }

    const unsigned char *data_;
    size_t size_, at_;
    GzipDevice *dev_;
    Tuning tune_;
    State state_ = Header;
    uint64_t bit_ = 0, edge_ = ~uint64_t(0);    // the deflate stream's next bit; where zlib hands back to the device
    uint32_t crc_ = 0;
    uint64_t isize_ = 0, zlibBytes_ = 0;
    int histMode_ = kGzipHistoryEmpty;
    std::vector<unsigned char> hist_;
    z_stream z_;
    bool zOn_ = false;
    size_t zNext_ = 0;                          // the next input byte zlib has not been given
    std::vector<char> out_;
};

}  // namespace detail
}  // namespace teloscope_mi355x
#endif
