"""benchlib.contigs — the assembly scan of bench.py: the synthetic assembly, the N = 1 and N > 1 steps, the sub-records of the line."""
from . import common
from .common import *  # noqa: F401,F403  (the standard modules bench.py always imported, and its constants)
from .verify import compare_sharded_with_single_gpu, verify_full_size


# ------------------------------------------------------------------------------------------- synthetic data
def contig_lengths(total, n, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    raw = np.exp(rng.uniform(np.log(1e6), np.log(250e6), size=n))
    lens = np.maximum((raw * (total / raw.sum())).astype(np.int64), 20000)
    lens[-1] += total - lens.sum()
    return [int(x) for x in lens]


def fill_synthetic(buf, offsets, lens, seed, dev):
    """Random ACGT + telomeres/TVRs at both ends of every contig + ITS blocks + N-runs + soft-masking,
    generated on the device (model of src/get-mock-chr.cpp:96-136).  Deterministic in (seed, lens): every rank
    of a sharded run generates the same assembly."""
    import numpy as np
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    chunk = 1 << 28
    for a in range(0, buf.numel(), chunk):
        b = min(buf.numel(), a + chunk)
        idx = torch.randint(0, 4, (b - a,), dtype=torch.uint8, device=dev, generator=g)
        buf[a:b] = lut[idx.long()]
        m = torch.rand(b - a, device=dev, generator=g) < 0.001          # 0.1 % lower case
        buf[a:b] |= (m.to(torch.uint8) << 5)
        del idx, m
    rng = np.random.default_rng(seed + 1)

    def tract(unit, reps, rate):
        t = np.tile(np.frombuffer(unit, dtype=np.uint8), reps).copy()
        k = rng.random(len(t)) < rate
        t[k] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(k.sum()))]
        return torch.from_numpy(t).to(dev)

    for off, n in zip(offsets, lens):
        p = torch.cat([tract(b"CCCTAA", 2000, 0.0), tract(b"CCCTAA", 100, 1.0 / 6)])
        q = torch.cat([tract(b"TTAGGG", 100, 1.0 / 6), tract(b"TTAGGG", 2000, 0.0)])
        if len(p) + len(q) < n:
            buf[off:off + len(p)] = p
            buf[off + n - len(q):off + n] = q
    n_its = 50
    for _ in range(n_its):
        ci = int(rng.integers(0, len(lens)))
        ln = int(rng.integers(200, 2000)) // 6
        unit = b"TTAGGG" if rng.random() < 0.5 else b"CCCTAA"
        at = int(rng.integers(20000, max(20001, lens[ci] - 20000 - 6 * ln)))
        t = tract(unit, ln, 0.02)
        buf[offsets[ci] + at:offsets[ci] + at + len(t)] = t
    for ci in rng.choice(len(lens), size=max(1, len(lens) // 100), replace=False):    # 1 % of contigs: an N-run
        ln = int(rng.integers(100, 10001))
        at = int(rng.integers(20000, max(20001, lens[ci] - 20000 - ln)))
        buf[offsets[ci] + at:offsets[ci] + at + ln] = ord("N")


def traffic_from_profile(args):
    """HBM bytes per launch from the committed rocprofv3 PMC passes of the default command, with where it came
    from; null when the kernel source is newer than the profile (a stale figure is worse than none)."""
    if args.gbases != 3.0 or args.contigs != 200 or args.flags != FLAGS:
        return None, None
    best = None
    pdir = os.path.join(ROOT, "profiles")
    for rd in sorted(os.listdir(pdir)) if os.path.isdir(pdir) else []:
        cand = os.path.join(pdir, rd, "pmc_traffic.json")
        if os.path.exists(cand):
            best = cand
    if best is None:
        return None, None
    d = json.load(open(best))
    src = "static: %s" % os.path.relpath(best, ROOT)
    want = d.get("kernels_hip_sha256")
    if want:
        import hashlib
        have = hashlib.sha256(open(os.path.join(ROOT, "teloscope_amd", "csrc", "kernels.hip"), "rb").read()).hexdigest()
        if have != want:
            return None, src + " is stale (kernels.hip changed since it was measured)"
        src += " @ kernels.hip sha256 %s" % want[:12]
    else:
        return None, src + " carries no kernel hash (measured for an earlier kernel)"
    return d["hbm_bytes_per_launch"], src


def fastest_box_seen(args):
    """Kernel time (ms) of the default workload on the fastest box the current kernels.hip has been measured on, from the committed
    profile that carries its hash; None for another workload or a newer kernel."""
    nbytes, src = traffic_from_profile(args)
    if nbytes is None or not src:
        return None
    path = os.path.join(ROOT, src.split("static: ", 1)[1].split(" @", 1)[0])
    try:
        return float(json.load(open(path)).get("fastest_box_seen", {}).get("kernel_ms")) or None
    except (OSError, TypeError, ValueError):
        return None


# ------------------------------------------------------------------------------------------- CPU baseline
def cpu_baseline(args, opts, buf, offsets, lens):
    """Bounded sample of the same workload on the host cores through the oracle port, with the reference's own
    parallel decomposition: one job per path (src/input.cpp:719-724), here one contig slice per thread (ctypes
    releases the GIL inside the C call); at 1 thread and at as many threads as the process may use, best of 3 each
    (BASELINE.md section 3).  The process was bound to the GPU's NUMA node for the PCIe legs: for this leg it gets back every
    CPU it was started with.  The reference binary itself cannot be built (gfalibs is absent from the reference tree and
    stand-in headers are not allowed), so this port is not calibrated against it."""
    from concurrent.futures import ThreadPoolExecutor
    from tests.backends import OracleBackend
    bound = os.sched_getaffinity(0)
    if common.ORIG_AFFINITY:
        os.sched_setaffinity(0, common.ORIG_AFFINITY)
    try:
        n = len(lens)
        ncpu = len(os.sched_getaffinity(0))
        cores = max(1, min(ncpu, n))
        # ~10-30 s of CPU work in all (three passes at N threads + three single-core passes), whatever the core count
        total_sample = args.cpu_sample_mb * 1e6 * max(1.0, cores / 4.0) / 4.0
        per_job = int(total_sample / cores)
        order = sorted(range(n), key=lambda i: -lens[i])[:cores]
        jobs = []
        for ci in order:
            nb = int(min(per_job, lens[ci]))
            jobs.append(buf[offsets[ci]:offsets[ci] + nb].cpu().numpy().tobytes().upper())
        backends = [OracleBackend(opts) for _ in jobs]

        def run(i):
            return backends[i].oracle.bench_scan(jobs[i])

        t1 = tn = None
        with ThreadPoolExecutor(max_workers=cores) as ex:
            for _ in range(3):
                c0 = time.perf_counter()
                r1 = run(0)                                         # one core, one job
                d = time.perf_counter() - c0
                t1 = d if t1 is None else min(t1, d)
                c0 = time.perf_counter()
                res = list(ex.map(run, range(len(jobs))))
                d = time.perf_counter() - c0
                tn = d if tn is None else min(tn, d)
        took = sum(len(j) for j in jobs)
        assert r1[0] == res[0][0]
        return {"value": round(took / tn / 1e9, 5), "unit": "Gbases/s", "cores": cores, "host_cpus": os.cpu_count(), "cpus_usable": ncpu,
                "kind": "port", "single_core_value": round(len(jobs[0]) / t1 / 1e9, 5), "passes": "best of 3 at 1 thread and at %d threads" % cores,
                "calibrated_against_reference": False,
                "sample": "first %.0f Mb of each of the %d largest contigs of the same synthetic assembly "
                          "(%.0f Mb), same flags, scan stage only incl. block calling "
                          "(oracle/teloscope_oracle.c: trie walk + carry loop), one job per contig as the "
                          "reference's -j N does, on every CPU the process was started with; %d windows, %d matches, best pass "
                          "%.1f s wall (%.1f s for one job on one core); the reference binary cannot be built here (gfalibs "
                          "absent), so the port is not calibrated against it" % (per_job / 1e6, len(jobs), took / 1e6, sum(r[1] for r in res),
                                                                                  sum(r[2] for r in res), tn, t1)}
    finally:
        os.sched_setaffinity(0, bound)


def pcie_inclusive(L, K, tel, buf, offsets, lens, total):
    """ASCII in host memory in, results in host memory out, through the drop-in entry points (pipelined upload,
    scan, block calling, D2H, host post-processing) — SURVEY 8d's second figure; reported beside `value`, never
    in it."""
    n = len(lens)
    import mmap
    import numpy as np
    import torch
    # the caller's buffer: ordinary pageable memory.  (TS_BENCH_HOST_HUGEPAGES=1 puts it on 2 MB pages when the kernel grants
    # them on request — measured: no difference, 84 against 84 Gbases/s.)
    nbytes = int(buf.numel())
    host_pages = "4 KB pages"
    if os.environ.get("TS_BENCH_HOST_HUGEPAGES", "0") == "1" and hasattr(mmap, "MADV_HUGEPAGE"):
        mm = mmap.mmap(-1, nbytes + (4 << 20))
        try:
            mm.madvise(mmap.MADV_HUGEPAGE)
            host_pages = "anonymous mapping with madvise(MADV_HUGEPAGE)"
        except OSError:
            pass
        whole = np.frombuffer(mm, dtype=np.uint8)
        skip = (-whole.ctypes.data) % (2 << 20)
        host = whole[skip:skip + nbytes]
        torch.from_numpy(host).copy_(buf)
    else:
        host = buf.cpu().numpy()
    segs = (K.SegmentIn * n)()
    base = host.ctypes.data
    for i in range(n):
        segs[i].seq = C.cast(C.c_void_p(base + offsets[i]), C.c_char_p)
        segs[i].len = lens[i]
        segs[i].abs_pos = 0
        segs[i].tips_only = 0
    e2e = {}
    for name, with_matches in (("blocks_windows_counts", False), ("with_match_vectors", True)):
        res = (K.SegmentOut * n)()
        cnts = (K.SegmentCounts * n)()
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            rc = (L.ts_scan_segments(tel._ctx.ptr, segs, n, res) if with_matches
                  else L.ts_scan_segments_blocks(tel._ctx.ptr, segs, n, res, cnts))
            dt = time.perf_counter() - t0
            if rc != 0:
                raise RuntimeError(tel._ctx.error())
            nm = int(sum(res[i].n_matches for i in range(n))) if with_matches else int(sum(c.n_matches for c in cnts))
            L.ts_free_segments(res, n)
            best = dt if best is None else min(best, dt)
        e2e[name] = {"seconds": round(best, 4), "gbases_per_s": round(total / best / 1e9, 3), "matches": nm}
    # the same call with the bases handed over ALREADY packed (TS_INPUT_PACKED2: 2-bit codes + invalid runs): what a front end
    # that packs while it parses passes (a FASTA reader touches every base once anyway) — the library's staging threads then
    # copy a quarter of the bytes instead of reading 3 GB of ASCII, which is what bounds the legs above.  The packing itself
    # (ts_pack_bases, here on a thread per contig, untimed) is the front end's pass over the text, not this entry point's.
    if int(L.ts_takes_text_input(tel._ctx.ptr, 0)):
        from concurrent.futures import ThreadPoolExecutor
        packed, keep = [None] * n, [None] * n

        def pack_one(i):
            m = int(lens[i])
            codes = np.zeros((m + 3) // 4 + 64, dtype=np.uint8)
            runs = []
            piece = 1 << 28
            for a in range(0, m, piece):
                mm_ = min(piece, m - a)
                cap = 1 << 16
                while True:
                    rr = np.zeros((cap, 2), dtype=np.uint32)
                    nr = C.c_uint64(0)
                    rc = L.ts_pack_bases(C.cast(C.c_void_p(base + offsets[i] + a), C.c_char_p), mm_, int(bool(tel.userInput.foldCase)),
                                         C.c_void_p(codes.ctypes.data + a // 4), C.c_void_p(rr.ctypes.data), cap, C.byref(nr))
                    if rc == 0:
                        break
                    if int(nr.value) <= cap:
                        raise RuntimeError("ts_pack_bases failed")
                    cap = int(nr.value) + 16
                for s0, ln in rr[:int(nr.value)]:
                    runs.append((a + int(s0), int(ln)))
            arr = (K.PackedRun * max(1, len(runs)))()
            for q, (s0, ln) in enumerate(runs):
                arr[q].start, arr[q].len = s0, ln
            packed[i] = K.PackedSeq(C.c_void_p(codes.ctypes.data), C.cast(arr, C.c_void_p), len(runs))
            keep[i] = (codes, arr)

        with ThreadPoolExecutor(max_workers=8) as ex:
            list(ex.map(pack_one, range(n)))
        psegs = (K.SegmentIn * n)()
        for i in range(n):
            psegs[i].seq = C.cast(C.pointer(packed[i]), C.c_char_p)
            psegs[i].len = lens[i]
            psegs[i].input_format = K.TS_INPUT_PACKED2
        res = (K.SegmentOut * n)()
        cnts = (K.SegmentCounts * n)()
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            rc = L.ts_scan_segments_blocks(tel._ctx.ptr, psegs, n, res, cnts)
            dt = time.perf_counter() - t0
            if rc != 0:
                raise RuntimeError(tel._ctx.error())
            nm = int(sum(c.n_matches for c in cnts))
            L.ts_free_segments(res, n)
            best = dt if best is None else min(best, dt)
        if nm != e2e["blocks_windows_counts"]["matches"]:
            raise RuntimeError("packed input and ASCII input gave different match counts")
        e2e["blocks_windows_counts_packed_in"] = {
            "seconds": round(best, 4), "gbases_per_s": round(total / best / 1e9, 3), "matches": nm,
            "input": "TS_INPUT_PACKED2: 2-bit codes + invalid runs in host memory (%.2f GB instead of %.2f), packed before the clock "
                     "starts as a FASTA front end would while parsing" % (total / 4e9, total / 1e9)}
        del packed, keep, psegs
    # FASTA TEXT in (TS_INPUT_TEXT_PIECES): the assembly as 80-column FASTA lines in host memory — what a front end that maps a file
    # holds — handed over as text pieces; the library's staging threads skip the line ends and pack INSIDE the clock.  This is the
    # honest "file bytes in host memory -> results" figure (round 4's verdict, item 4); the packed-in leg above leaves the packing out.
    if int(L.ts_takes_text_input(tel._ctx.ptr, 0)) and not os.environ.get("TS_BENCH_NO_TEXT_IN"):
        width, lines_per_piece = 80, 200_000                              # 16.2 MB of text per piece (the format's limit: 16 MiB)
        texts, piece_arrays, tsegs = [], [], (K.SegmentIn * n)()
        for i in range(n):
            m = int(lens[i])
            bases = host[offsets[i]:offsets[i] + m]
            rows = m // width
            txt = np.empty(m + rows + (1 if m % width else 0), dtype=np.uint8)
            if rows:
                body = txt[:rows * (width + 1)].reshape(rows, width + 1)
                body[:, :width] = bases[:rows * width].reshape(rows, width)
                body[:, width] = 10
            if m % width:
                txt[rows * (width + 1):-1] = bases[rows * width:]
                txt[-1] = 10
            texts.append(txt)
            step_t, step_b = lines_per_piece * (width + 1), lines_per_piece * width
            npieces = max(1, -(-len(txt) // step_t))
            arr = (K.TextPiece * npieces)()
            for q in range(npieces):
                t0_, t1_ = q * step_t, min(len(txt), (q + 1) * step_t)
                arr[q].text = C.cast(C.c_void_p(txt.ctypes.data + t0_), C.c_char_p)
                arr[q].text_len = t1_ - t0_
                arr[q].n_bases = min(m, (q + 1) * step_b) - q * step_b
            piece_arrays.append(arr)
            tsegs[i].seq = C.cast(arr, C.c_char_p)
            tsegs[i].len = m
            tsegs[i].input_format = K.TS_INPUT_TEXT_PIECES
            tsegs[i].n_pieces = npieces
        res = (K.SegmentOut * n)()
        cnts = (K.SegmentCounts * n)()
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            rc = L.ts_scan_segments_blocks(tel._ctx.ptr, tsegs, n, res, cnts)
            dt = time.perf_counter() - t0
            if rc != 0:
                raise RuntimeError(tel._ctx.error())
            nm = int(sum(c.n_matches for c in cnts))
            L.ts_free_segments(res, n)
            best = dt if best is None else min(best, dt)
        if nm != e2e["blocks_windows_counts"]["matches"]:
            raise RuntimeError("FASTA text input and joined bases gave different match counts")
        e2e["fasta_text_in"] = {
            "seconds": round(best, 4), "gbases_per_s": round(total / best / 1e9, 3), "matches": nm,
            "input": "TS_INPUT_TEXT_PIECES: %d-column FASTA lines in host memory (%.2f GB of text), pieces of %d lines; line ends skipped and "
                     "bases packed by the library's staging threads inside the clock" % (width, sum(len(t) for t in texts) / 1e9, lines_per_piece)}
        del texts, piece_arrays, tsegs
    # the writers' view over ts_scan_segments_multi: one shard per context, each over its own PCIe link (here: the contexts
    # this one GPU can give — the figure says what the entry point costs, not what more links would add)
    import teloscope_amd as ta
    n_ctx = max(1, min(int(os.environ.get("TS_BENCH_CTXS", "1")), 8))
    tels = [tel] + [ta.Teloscope(tel.userInput) for _ in range(n_ctx - 1)]
    ctxs = (C.c_void_p * n_ctx)(*[t._ctx.ptr for t in tels])
    res = (K.SegmentOut * n)()
    cnts = (K.SegmentCounts * n)()
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        rc = L.ts_scan_segments_multi(ctxs, n_ctx, segs, n, res, cnts)
        dt = time.perf_counter() - t0
        if rc != 0:
            raise RuntimeError(tel._ctx.error())
        nvis = int(sum(res[i].n_matches for i in range(n)))
        nm = int(sum(c.n_matches for c in cnts))
        L.ts_free_segments(res, n)
        best = dt if best is None else min(best, dt)
    e2e["writer_view_multi"] = {"seconds": round(best, 4), "gbases_per_s": round(total / best / 1e9, 3), "matches": nm,
                                "visible_matches": nvis, "n_ctx": n_ctx,
                                "entry_point": "ts_scan_segments_multi (windows, blocks and the match records a writer reads; one shard per context)"}
    # the GENERAL path (parameter sets the tiled kernel does not take: here a mixed-length set, -p TTAGGG,TTAGG) over the same
    # host buffer and entry point — generic.hip's list kernel, block calling on the device, upload of group g + 1 beside group
    # g's kernels.  Reported beside the figures above, never in `value`; TS_BENCH_NO_GENERAL=1 skips it.
    if not os.environ.get("TS_BENCH_NO_GENERAL"):
        from teloscope_amd.cli import parse_cli, user_input
        # (the second and third: what round 4 sent to the host's block calling — a stream that is not in position order (lengths 6 and
        # 14 under w > s), and the wide form (nine lengths: beyond the table forms); the device writes such a stream in the
        # reference's push order and calls the blocks over it)
        for key, gflags, what in (
                ("general_path_blocks_windows_counts", "-p TTAGGG,TTAGG -w 1000 -s 500 -r -g -e -m -i",
                 "generic.hip: ts_general_fused_list, blockcall.hip over the records in the tiles' slots (stream in position order)"),
                ("general_path_push_order_blocks_windows_counts", "-p TTAGGG,TTTAGGGTTTAGGG -x 0 -w 1000 -s 500 -r -g -e -m -i",
                 "generic.hip: ts_general_fused_list + ts_general_compact_push (stream in the reference's push order), blockcall.hip MODE 1"),
                ("general_path_wide_blocks_windows_counts", "-x 0 -p TTAG,TTAGG,TTAGGG,TTTAGGG,TTTTAGGG,TTAGGGTTA,TTAGGGTTAG,TTAGGGTTAGG,TTAGGGTTAGGG -w 1000 -s 500 -r -g -e -m -i",
                 "generic.hip: ts_general_wide + ts_general_compact_push, blockcall.hip MODE 1 (wide records)")):
            gtel = ta.Teloscope(user_input(parse_cli("x.fa " + gflags), device=tel.userInput.device))
            if not gtel.usesFastPath():
                res = (K.SegmentOut * n)()
                cnts = (K.SegmentCounts * n)()
                best = None
                for _ in range(3):
                    t0 = time.perf_counter()
                    rc = L.ts_scan_segments_blocks(gtel._ctx.ptr, segs, n, res, cnts)
                    dt = time.perf_counter() - t0
                    if rc != 0:
                        raise RuntimeError(gtel._ctx.error())
                    nm = int(sum(c.n_matches for c in cnts))
                    nb = int(sum(res[i].n_terminal_blocks + res[i].n_interstitial_blocks for i in range(n)))
                    L.ts_free_segments(res, n)
                    best = dt if best is None else min(best, dt)
                e2e[key] = {"flags": gflags, "patterns": len(gtel.userInput.patternInfo), "seconds": round(best, 4),
                            "gbases_per_s": round(total / best / 1e9, 3), "matches": nm, "blocks": nb, "kernels": what}
            gtel.close()
    return {"entry_points": "ts_scan_segments_blocks / ts_scan_segments (pageable host buffers in, host results out; "
                            "groups of ~512 MB pipelined through upload / scan / download stages; bases cross PCIe as 2-bit codes + invalid runs, packed by the staging threads and unpacked on the device; best of 3)", "host_buffer": host_pages, "n_ctx": 1, **e2e}


# ------------------------------------------------------------------------------------------- the assembly scan
DUMP_WINDOWS = 400_000          # window records in the --dump-outputs sample (9 columns of float64: 28.8 MB)
DUMP_MATCHES = 500_000          # match records in it (5 columns: 20 MB)


def dump_scan_outputs(path, L, K, tel, plan, batch, dev, sptr):
    """--dump-outputs of the assembly scan: what a caller of the timed scan reads back from its last step, as float64
      segment_summary.npy  [segments, 4]  windows, matches, canonical, forward per segment (ts_batch_segment_summary)
      windows.npy          [k, 9]  a seeded sample of the window records: window index, then A, C, G, T and the canonical /
                                   non-canonical / forward / reverse covered bases (ts_batch_windows_ptr)
      matches.npy          [k, 5]  a seeded sample of the match records in position order (ts_batch_export): record index,
                                   segment, position in the segment, forward, canonical
    Untimed; the batch must have been synced after its last scan."""
    import numpy as np
    import torch
    info = K.BatchInfo()
    L.ts_batch_get_info(batch, C.byref(info))
    n_seg, n_win, n_tiles = int(info.n_segments), int(info.n_windows), int(info.n_tiles)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def device_copy(src_ptr, n_u32):
        t = torch.empty(max(1, n_u32), dtype=torch.int32, device=dev)
        if n_u32:
            assert hip.hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(src_ptr), C.c_size_t(4 * n_u32), 3) == 0
            # (a device-to-device hipMemcpy may return before the copy is done, and torch's stream does not wait for it)
            torch.cuda.synchronize()
        return t[:n_u32]

    torch.cuda.synchronize()
    summ = torch.zeros(n_seg * 4, dtype=torch.int64, device=dev)
    dense = torch.empty(int(info.n_matches) + 1024, dtype=torch.int32, device=dev)
    total = torch.zeros(2, dtype=torch.int64, device=dev)
    if (L.ts_batch_segment_summary(batch, C.c_void_p(summ.data_ptr()), sptr) != 0
            or L.ts_batch_export(batch, C.c_void_p(dense.data_ptr()), dense.numel(), C.c_void_p(total.data_ptr()), sptr) != 0):
        raise RuntimeError(tel._ctx.error())
    torch.cuda.synchronize()
    n_rec, incomplete = (int(x) for x in total.tolist())
    if incomplete or n_rec != int(info.n_matches):
        raise RuntimeError("--dump-outputs: the exported match stream holds %d of %d records (incomplete: %d)"
                           % (n_rec, int(info.n_matches), incomplete))

    wins = device_copy(L.ts_batch_windows_ptr(batch), 8 * n_win).view(-1, 8)
    wi = dump_sample_index(n_win, DUMP_WINDOWS)
    w = wins[torch.from_numpy(wi).to(dev)].cpu().numpy().view(np.uint32)
    windows = np.concatenate([wi[:, None].astype(np.float64), w.astype(np.float64)], axis=1)
    del wins

    stats = device_copy(L.ts_batch_tile_stats_ptr(batch), 4 * n_tiles).view(-1, 4).cpu().numpy().view(np.uint32)
    offs = np.concatenate(([0], np.cumsum(stats[:, 0].astype(np.int64))))
    assert int(offs[-1]) == n_rec, (int(offs[-1]), n_rec)
    mi = dump_sample_index(n_rec, DUMP_MATCHES)
    rec = dense[torch.from_numpy(mi).to(dev)].cpu().numpy().view(np.uint32).astype(np.int64)
    del dense
    tiles = plan.tiles
    tile = np.searchsorted(offs, mi, side="right") - 1
    matches = np.stack([mi, tiles["seg_index"][tile].astype(np.int64), tiles["seg_offset"][tile].astype(np.int64) + (rec >> 2),
                        (rec >> 1) & 1, rec & 1], axis=1).astype(np.float64)
    write_dump(path, {"segment_summary": summ.view(n_seg, 4).cpu().numpy().astype(np.float64),
                      "windows": windows, "matches": matches})


def run_scan(args, rank, local_rank, world, dev, backend):
    import numpy as np
    import torch
    import torch.distributed as dist
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from teloscope_amd import distributed as D
    from teloscope_amd.cli import parse_cli, user_input

    opts = parse_cli("x.fa " + args.flags)
    ui = user_input(opts, device=dev.index)
    tel = ta.Teloscope(ui)
    L = K.lib()
    forced_strong = world == 1 and bool(os.environ.get("TS_BENCH_FORCE_STRONG"))
    strong = (world > 1 or forced_strong) and not args.weak
    if args.dump_outputs and strong:
        raise SystemExit("bench.py: --dump-outputs writes the outputs of the single-GPU scan, not of the sharded path")
    total = int(args.gbases * 1e9)
    lens = contig_lengths(total, args.contigs, 42 + (rank if args.weak else 0))
    n = len(lens)
    plan = D.ShardPlan(tel, lens, world=world if strong else 1)
    offsets = plan.segment_offsets()
    info = plan.info
    # The scans run on a stream of their own, not on the null stream: work on the null stream does not overlap with work on
    # other streams the way two ordinary streams overlap (the sharded step at the size of one of 8 ranks: 0.349 -> 0.283 ms
    # with block calling + packing of step i beside the scan of step i + 1).
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    stream = torch.cuda.current_stream()
    sptr = C.c_void_p(stream.cuda_stream)
    xdev = dev if backend == "nccl" else torch.device("cpu")

    # the assembly: generated whole on every rank (same seed -> same bytes); a strong-scaling rank keeps only
    # the bytes its tile range reads
    full = torch.zeros(int(info.input_bytes), dtype=torch.uint8, device=dev)
    fill_synthetic(full, offsets, lens, 42 + (rank if args.weak else 0), dev)
    keep_full = (not strong) or rank == 0                       # (rank 0 checks the merged messages against its own scan of the whole assembly)
    buf = full                                                  # (a strong-scaling rank cuts its own range out below)
    sharded = None

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        t = torch.tensor([x], dtype=torch.float64, device=xdev)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def every_rank_s(x):
        t = torch.tensor([x], dtype=torch.float64, device=xdev)
        if world == 1:
            return [float(x)]
        got = [torch.zeros(1, dtype=torch.float64, device=xdev) for _ in range(world)]
        dist.all_gather(got, t)
        return [float(g.item()) for g in got]

    enqueue_s = [0.0]
    own_s = [0.0]

    def timed(step_fn, drain_fn, nsteps):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        barrier()
        t0 = time.perf_counter()
        ev0.record(stream)
        for i in range(nsteps):
            step_fn(i)
        enqueue_s[0] = time.perf_counter() - t0                 # host time to ENQUEUE the steps (nothing waited for)
        drain_fn()
        ev1.record(stream)
        torch.cuda.synchronize()
        own_s[0] = time.perf_counter() - t0                     # this rank's own steps done (before it waits for the others)
        barrier()
        elapsed = time.perf_counter() - t0
        return max_over_ranks(elapsed), ev0.elapsed_time(ev1) / max(1, nsteps)

    # A device that has just been handed its first kernels is not in its steady state: the launch time of this kernel rises
    # for five launches (0.81 -> 0.97 ms) and then falls for about forty (-> 0.765 ms; profiles/r02/launch_ramp.txt).  The W
    # warm-up steps of the contract are taken from there: SETTLE_LAUNCHES untimed scans first (reported in config.settle).
    def settle(step_fn, drain_fn):
        for n in range(SETTLE_LAUNCHES):
            step_fn(n)
            if n % 8 == 7:
                drain_fn()
        drain_fn()
        torch.cuda.synchronize()
        settle_info["launches"] = SETTLE_LAUNCHES

    settle_info = {"launches": 0}
    out = None
    if not strong:
        # ---------------------------------------------------------------- N = 1 (or weak scaling)
        batch = plan.batch
        if os.environ.get("TS_BENCH_EMIT") == "1":          # A/B: the plain scan with the emitting build (ts_batch_set_emit)
            L.ts_batch_set_emit(batch, 1)
        dptr = C.c_void_p(buf.data_ptr())
        summaries = [torch.zeros(n * 4, dtype=torch.int64, device=dev) for _ in range(2)]
        gathered = [[torch.zeros(n * 4, dtype=torch.int64, device=xdev) for _ in range(world)]
                    if (world > 1 and rank == 0) else None for _ in range(2)]
        pending = [None, None]

        def step(i):
            if L.ts_batch_scan(batch, dptr, sptr) != 0:
                raise RuntimeError(tel._ctx.error())
            if world > 1:                                       # weak scaling: per-segment hit summaries to rank 0
                j = i & 1
                if pending[j] is not None:
                    pending[j].wait()
                if L.ts_batch_segment_summary(batch, C.c_void_p(summaries[j].data_ptr()), sptr) != 0:
                    raise RuntimeError(tel._ctx.error())
                src = summaries[j] if backend == "nccl" else summaries[j].cpu()
                pending[j] = dist.gather(src, gathered[j], dst=0, async_op=True)

        def drain():
            for j in range(2):
                if pending[j] is not None:
                    pending[j].wait()
                    pending[j] = None

        # what a user sees: a genome is scanned ONCE.  The first scan of the process (device buffers allocated, code objects
        # loaded), the second (a single shot on a warm library), and the contract's own protocol without the settling scans
        # below (W warm-ups, then K steps) are measured before the steady state that `value` reports.
        protocol = {}
        if world == 1 and not args.full:
            # a plain run skips those figures; its first scan is still followed by a sync, as theirs is
            step(0)
            drain()
            if L.ts_batch_sync(batch) != 0:      # (grows the match buffer and rescans if the first scan overflowed)
                raise RuntimeError(tel._ctx.error())
        elif world == 1:
            def one():
                torch.cuda.synchronize()
                c0 = time.perf_counter()
                step(0)
                drain()
                torch.cuda.synchronize()
                return (time.perf_counter() - c0) * 1e3
            protocol["first_scan_ms_incl_module_load_and_allocation"] = round(one(), 3)
            if L.ts_batch_sync(batch) != 0:      # (grows the match buffer and rescans if the first scan overflowed)
                raise RuntimeError(tel._ctx.error())
            protocol["single_shot_ms"] = round(one(), 4)
            for i in range(args.warmup):
                step(i)
            drain()
            torch.cuda.synchronize()
            c0 = time.perf_counter()
            for i in range(args.steps):
                step(i)
            drain()
            torch.cuda.synchronize()
            protocol["after_%d_warmups_ms_per_step" % args.warmup] = round((time.perf_counter() - c0) / args.steps * 1e3, 4)
        settle(step, drain)
        for i in range(args.warmup):
            step(i)
        drain()
        if L.ts_batch_sync(batch) != 0:          # also grows the match buffer if it overflowed
            raise RuntimeError(tel._ctx.error())
        tmax, dev_ms = timed(step, drain, args.steps)
        if protocol:
            protocol["settled_ms_per_step"] = round(tmax / args.steps * 1e3, 4)
            protocol["value_is"] = "settled_ms_per_step: the steady state after %d untimed scans; a genome scanned once costs single_shot_ms" % SETTLE_LAUNCHES
        if L.ts_batch_sync(batch) != 0:
            raise RuntimeError(tel._ctx.error())
        L.ts_batch_get_info(batch, C.byref(info))
        kern_ms, launches = float(info.avg_kernel_ms), int(info.kernel_launches)
        if args.dump_outputs:
            dump_scan_outputs(args.dump_outputs, L, K, tel, plan, batch, dev, sptr)
        alg_bytes, n_matches, n_windows, n_tiles = int(info.algorithmic_bytes), int(info.n_matches), int(info.n_windows), int(info.n_tiles)
        result_batch = batch
        extra_cfg = {"timed_region": "resident ASCII in HBM -> window records + packed match stream in HBM"
                                     + (" + RCCL gather of per-segment hit summaries (weak scaling: every rank its own assembly)"
                                        if world > 1 else "")}
        if protocol:
            extra_cfg["launch_protocol"] = protocol
        bases_done = world * total
    elif not args.full_exchange:
        # ---------------------------------------------------------------- N > 1, strong scaling (configs[2]): shard results
        # Every rank scans its tile range (+ context tiles), calls its blocks on its own device and packs ONE message of a
        # size both sides know from the plan; one grouped send / recv per step brings the messages to rank 0.  Nothing is
        # read back to the host inside a step; the messages' headers are checked (and the messages merged on the host,
        # ts_shards_finalize) before the timed steps and after them.
        slots = max(2, int(os.environ.get("TS_BENCH_SLOTS", "4")))      # (profiles/r04/hwq_sweep.txt, slots_sweep.txt)
        scale = 1
        exch = D.ShardExchange(plan, rank, dev, dst=0, slots=slots, scale=scale)
        shard = D.PackedShard(plan, rank, dev, slots=slots, scale=scale)
        # one scan in four of a slot is timed (roofline.kernel_ms is their mean): the start event of a timed scan is a packet on
        # the scan's queue, 0.005 ms per scan at the N = 8 size (profiles/r05/shard_step_queues.txt)
        shard.set_timing(max(0, int(os.environ.get("TS_BENCH_TIME_EVERY", "4"))))
        buf = full[int(shard.info.input_begin):max(int(shard.info.input_end), int(shard.info.input_begin) + 64)].clone()
        if not keep_full:
            del full
            torch.cuda.empty_cache()
        in_ptr = buf.data_ptr()
        pending = [None] * slots
        # Streams: block calling + packing of step i (no LDS, few registers) run beside the scans of the steps after it (a
        # persistent kernel that holds every CU's LDS but leaves a SIMD room for one or two waves of anything else: the
        # pack kernels are chains of latency, they make progress at that occupancy but take about two scans to finish —
        # hence THREE buffer slots and TWO pack streams, so that two packs are in flight beside the scan), and the transfer
        # of step i's message beside all of it.  A slot's scan waits for the pack that last read its records; a slot's pack
        # waits for the transfer that last read its message.
        # (HIP maps streams onto four hardware queues and two streams on one queue take turns: the pack streams are chosen so that
        # they do not share the scan stream's — distributed.concurrent_streams)
        pack_streams = D.concurrent_streams(tel, dev, 1 + max(1, int(os.environ.get("TS_BENCH_PACK_STREAMS", "2"))), first=stream)[1:]
        # (TS_BENCH_SCAN_STREAMS=2 alternates the scans of consecutive steps between two streams, so that the workgroups of
        # step i + 1 could take the CUs the tail of step i frees.  Measured, profiles/r04/two_scan_streams.txt: slower at every
        # size — 1.15 against 0.93 ms at 3 Gb, 0.188 against 0.177 at the N = 8 size: two persistent kernels that each want
        # every CU's whole LDS take turns badly.  One stream is the default.)
        scan_streams = [stream] + [torch.cuda.Stream(device=dev) for _ in range(max(1, int(os.environ.get("TS_BENCH_SCAN_STREAMS", "1"))) - 1)]
        packed = [torch.cuda.Event() for _ in range(slots)]
        used = [False] * slots
        # Rehearsal of the exchange's SHAPE on one GPU (TS_BENCH_REHEARSE_WORLD=8 with TS_BENCH_FORCE_STRONG=1): what rank 0 of
        # an N-rank job posts per step — one grouped batch of N - 1 receives, one per sender, of the message sizes the N-way
        # plan gives (ts_batch_shard_info) — and what the N - 1 senders post, all from this one rank on the real RCCL group
        # with itself as the peer: 2 (N - 1) operations per step in one batch_isend_irecv, `slots` steps in flight, posted
        # from the pack stream as in the real step.  What it cannot show is seven links; what it does show is the grouped
        # P2P call pattern of rank 0 meeting the library.  The received bytes are compared with what was sent afterwards.
        rehearse = None
        rw = int(os.environ.get("TS_BENCH_REHEARSE_WORLD", "0"))
        if world == 1 and rw > 1 and backend == "nccl":
            plan_r = D.ShardPlan(tel, lens, world=rw)
            sizes = [int(D.shard_info(plan_r, p).msg_bytes) for p in range(1, rw)]
            plan_r.close()
            gen = torch.Generator(device=dev)
            gen.manual_seed(7)
            rehearse = {"world": rw, "sizes": sizes,
                        "send": [[torch.randint(0, 256, (sz,), dtype=torch.uint8, device=dev, generator=gen) for sz in sizes] for _ in range(slots)],
                        "recv": [[torch.zeros(sz, dtype=torch.uint8, device=dev) for sz in sizes] for _ in range(slots)],
                        "posted": 0, "steps": 0}

        def post_rehearsal(j):
            ops = []
            for q in range(len(rehearse["sizes"])):
                ops.append(dist.P2POp(dist.irecv, rehearse["recv"][j][q], 0))
            for q in range(len(rehearse["sizes"])):
                ops.append(dist.P2POp(dist.isend, rehearse["send"][j][q], 0))
            rehearse["posted"] += len(ops)
            rehearse["steps"] += 1
            return dist.batch_isend_irecv(ops)

        def step(i):
            j = i % slots
            pack_stream = pack_streams[j % len(pack_streams)]
            scan_stream = scan_streams[i % len(scan_streams)]
            if used[j]:
                scan_stream.wait_event(packed[j])
            shard.scan(in_ptr, C.c_void_p(scan_stream.cuda_stream), j)
            with torch.cuda.stream(pack_stream):
                shard.wait_scan(C.c_void_p(pack_stream.cuda_stream), j)       # (the library's own event behind the scan)
                if pending[j] is not None:
                    for w in pending[j]:
                        w.wait()
                    pending[j] = None
                shard.pack(C.c_void_p(pack_stream.cuda_stream), j)
                packed[j].record(pack_stream)
                pending[j] = exch.post(shard.msgs[j], j) if rehearse is None else post_rehearsal(j)
            used[j] = True

        def drain():
            for j in range(slots):
                with torch.cuda.stream(pack_streams[j % len(pack_streams)]):
                    if pending[j] is not None:
                        for w in pending[j]:
                            w.wait()
                        pending[j] = None
            for ps in pack_streams + scan_streams[1:]:
                stream.wait_stream(ps)

        # ---- FIRST CONTACT (untimed), under a watchdog: one step taken apart — scan, pack, the grouped send / recv, each waited
        # for — before anything is pipelined.  On a real N-rank RCCL group this is the first time rank 0's N - 1 receives meet
        # N - 1 senders; a rank that never arrives would otherwise hang every rank (and the caller's clock) in the settling
        # loop below.  On time-out the rank prints which stage it was in and exits non-zero (Watchdog: os._exit, never an exec).
        first_contact = None
        if world > 1 or rehearse is not None or forced_strong:
            wd = Watchdog(float(os.environ.get("TS_BENCH_FIRST_EXCHANGE_TIMEOUT", "240")), rank,
                          "first exchange of %d rank(s) on %s" % (world, backend))
            c0 = time.perf_counter()
            wd.stage = "scan of this rank's tile range enqueued"
            shard.scan(in_ptr, sptr, 0)
            torch.cuda.synchronize()
            wd.stage = "block calling + pack enqueued"
            shard.pack(sptr, 0)
            torch.cuda.synchronize()
            n_ops = (world - 1) if rank == 0 else 1
            wd.stage = "posted %d grouped %s of %s bytes; waiting for them" % (
                n_ops, "receive(s) from ranks 1..%d" % (world - 1) if rank == 0 else "send to rank 0",
                [int(x.msg_bytes) for x in exch.infos[1:]] if rank == 0 else int(exch.infos[rank].msg_bytes))
            works = exch.post(shard.msgs[0], 0) if rehearse is None else post_rehearsal(0)
            for w in works:
                w.wait()
            torch.cuda.synchronize()
            wd.stage = "exchange complete; barrier"
            barrier()
            first_ms = (time.perf_counter() - c0) * 1e3
            # who arrived: rank 0 reads every part's header (a message that never came is all zeros: no magic, no part number)
            ranks_seen = None
            if rank == 0:
                ranks_seen = []
                for p, m in enumerate(exch.messages(shard.msgs[0], 0)):
                    st = K.ShardStatus()
                    if L.ts_shard_peek(m.ctypes.data, m.nbytes, C.byref(st)) == 0 and int(st.part) == p and int(st.n_parts) == world:
                        ranks_seen.append(p)
            wd.stage = "headers read on rank 0; broadcasting the verdict"
            seen_ok = max_over_ranks(0.0 if (rank != 0 or ranks_seen == list(range(world))) else 1.0) == 0.0
            wd.cancel()
            first_contact = {"ms": round(first_ms, 3), "ranks_seen": ranks_seen, "all_ranks_seen": seen_ok,
                             "what": "one step taken apart (scan, pack, grouped send / recv; each waited for) before anything is pipelined; "
                                     "watchdog %s s" % os.environ.get("TS_BENCH_FIRST_EXCHANGE_TIMEOUT", "240")}
            if not seen_ok:
                raise RuntimeError("first exchange: rank 0 holds valid messages of parts %s only (of %d)" % (ranks_seen, world))
        # the pipelined steps run under a (generous) deadline of their own: a hang there also ends with a line that says where
        run_wd = Watchdog(float(os.environ.get("TS_BENCH_RUN_TIMEOUT", "900")), rank, "pipelined sharded steps (%d ranks, %s)" % (world, backend)) \
            if (world > 1) else None
        if run_wd:
            run_wd.stage = "settling scans"
        settle(step, drain)
        for i in range(max(args.warmup, slots)):
            step(i)
        drain()
        torch.cuda.synchronize()
        if run_wd:
            run_wd.stage = "capacity / region settling (exch.check)"
        # capacities and record regions settle here (untimed): a scan that overflowed its regions is regrown, a message that
        # overflowed gets a larger scale on every rank; an input the shards' assumptions do not hold for takes the full exchange
        ok = False
        pre_timed_check = None
        for attempt in range(8):
            action, factor, merged = exch.check(shard.msgs[0], 0)
            if action == exch.OK and merged is not None and world > 1 and pre_timed_check is None:
                # ONE correctness pass before the clock starts: what the ranks' messages merge to against rank 0's own scan of
                # the whole assembly — every window record and every block, byte for byte
                if run_wd:
                    run_wd.stage = "rank 0: merged messages against its own single-GPU scan"
                one = D.ShardPlan(tel, lens, world=1)
                if L.ts_batch_scan(one.batch, C.c_void_p(full.data_ptr()), sptr) != 0 or L.ts_batch_sync(one.batch) != 0:
                    raise RuntimeError(tel._ctx.error())
                pre_timed_check = compare_sharded_with_single_gpu(L, K, tel, one.batch, {"seg_out": merged[1], "seg_cnt": merged[2]}, n, False)
                one.close()
            if merged is not None:
                D.free_segments(plan, merged[1])
            if action == exch.OK:
                ok = True
                break
            if action == exch.FULL:
                break
            if action == exch.SYNC:
                for j in range(slots):
                    shard.sync(j)
            elif action == exch.GROW:
                scale *= factor
                shard.set_scale(scale)
                exch.set_scale(scale)
            for i in range(slots):
                step(i)
            drain()
            torch.cuda.synchronize()
        if not ok:
            raise RuntimeError("the shard results need the full exchange for this input: run with --full-exchange")
        for j in range(slots):
            shard.kernel_ms(j)                                   # (harvest the scans' event times so far)
        if run_wd:
            run_wd.stage = "timed steps"
        tmax, dev_ms = timed(step, drain, args.steps)
        per_rank_ms = [round(x / args.steps * 1e3, 4) for x in every_rank_s(own_s[0])]
        if run_wd:
            run_wd.stage = "after the timed steps (step split, final check)"
        last = (args.steps - 1) % slots
        km = [shard.kernel_ms(j) for j in range(slots)]
        launches = sum(k[1] for k in km)
        kern_ms = sum(k[0] * k[1] for k in km) / max(1, launches)
        rinfo = km[last][2]
        alg_bytes = int(rinfo.algorithmic_bytes)
        # where a step's time goes when nothing overlaps: scan + pack / exchange, each waited for
        nb = min(10, args.steps)
        t_scan = t_pack = t_x = 0.0
        for i in range(nb):
            barrier()
            c0 = time.perf_counter()
            if L.ts_batch_scan(shard.batches[0], C.c_void_p(in_ptr), sptr) != 0:
                raise RuntimeError(tel._ctx.error())
            torch.cuda.synchronize()
            c1 = time.perf_counter()
            if L.ts_batch_pack_shard(shard.batches[0], C.c_void_p(shard.msgs[0].data_ptr()), shard.msgs[0].numel(), sptr) != 0:
                raise RuntimeError(tel._ctx.error())
            torch.cuda.synchronize()
            c2 = time.perf_counter()
            for w in exch.post(shard.msgs[0], 0):
                w.wait()
            torch.cuda.synchronize()
            c3 = time.perf_counter()
            t_scan += c1 - c0; t_pack += c2 - c1; t_x += c3 - c2
        split = {"scan_ms": round(max_over_ranks(t_scan / nb) * 1e3, 4), "block_calling_and_pack_ms": round(max_over_ranks(t_pack / nb) * 1e3, 4),
                 "exchange_ms": round(max_over_ranks(t_x / nb) * 1e3, 4), "steps": nb,
                 "note": "serialised (each phase waited for on the host); the timed region overlaps the exchange of step i "
                         "with the scan of step i+1"}
        # the last timed step's messages, checked and merged on rank 0 (untimed)
        action, factor, merged = exch.check(shard.msgs[last], last)
        if action != exch.OK:
            raise RuntimeError("a timed step's messages came out incomplete (action %d)" % action)
        result_batch = None
        n_windows, n_tiles = plan.n_windows, plan.n_tiles
        n_matches = 0
        sharded = None
        if rank == 0:
            rc_m, seg_out, seg_cnt = merged
            n_matches = int(sum(int(seg_cnt[i].n_matches) for i in range(n)))
            statuses = []
            for m in exch.messages(shard.msgs[last], last):
                st = K.ShardStatus()
                L.ts_shard_peek(m.ctypes.data, m.nbytes, C.byref(st))
                statuses.append(st)
            sharded = {"seg_out": seg_out, "seg_cnt": seg_cnt}
            extra_cfg = {"timed_region": "resident ASCII in HBM on %d ranks (consecutive tile ranges of ONE plan, + context tiles) -> scan + block calling "
                                         "on every rank's own device + ONE message per rank (bit-packed window records, the match records a writer "
                                         "reads, blocks) -> all messages in rank 0's HBM; no host synchronisation inside a step; the exchange of "
                                         "step i overlaps the scan of step i+1" % world,
                         "backend": backend + ("" if backend == "nccl" else " (rehearsal: ranks share a GPU, messages staged through the host)"),
                         "bases_per_rank": [int(x.bases) for x in exch.infos],
                         "exchange": {"bytes_over_links_per_step": exch.bytes_over_links,
                                      "message_bytes_per_rank": [int(x.msg_bytes) for x in exch.infos],
                                      "window_bytes": int(exch.infos[0].window_bytes), "visible_record_bytes": int(exch.infos[0].visible_bytes),
                                      "visible_records_per_rank": [int(st.n_visible) for st in statuses],
                                      "visible_capacity_per_rank": [int(st.visible_capacity) for st in statuses],
                                      "blocks_per_rank": [int(st.n_blocks) for st in statuses],
                                      "capacity_scale": scale, "context_tiles": int(exch.infos[0].context_tiles),
                                      "round2_full_exchange_bytes_over_links": None,
                                      "first_contact": first_contact,
                                      "ranks_seen": first_contact["ranks_seen"] if first_contact else None,
                                      "merged_equals_single_gpu_scan_before_timed_steps": pre_timed_check},
                         "per_rank_ms_per_step": per_rank_ms,
                         "step_split": split}
            if rehearse is not None:
                torch.cuda.synchronize()
                same = all(torch.equal(rehearse["recv"][j][q], rehearse["send"][j][q])
                           for j in range(min(slots, rehearse["steps"])) for q in range(len(rehearse["sizes"])))
                if not same:
                    raise RuntimeError("exchange rehearsal: received bytes differ from the bytes sent")
                extra_cfg["exchange"]["rehearsal"] = {
                    "of_world": rehearse["world"], "posted_ops_per_step": rehearse["posted"] // max(1, rehearse["steps"]),
                    "steps_posted": rehearse["steps"], "bytes_per_step": int(sum(rehearse["sizes"])),
                    "message_bytes": rehearse["sizes"], "received_equals_sent": True,
                    "what": "rank 0's grouped batch of an %d-rank step (N - 1 receives) plus the N - 1 sends, from ONE rank on the RCCL "
                            "group with itself as the peer, `slots` steps in flight" % rehearse["world"]}
        else:
            extra_cfg = {}
        if run_wd:
            run_wd.cancel()
        bases_done = total
    else:
        # ---------------------------------------------------------------- N > 1, strong scaling, round 2's full exchange
        r = plan.ranges[rank]
        buf = full[r.input_begin:r.input_end].clone()
        if not keep_full:
            del full
            torch.cuda.empty_cache()
        sharded = None
        slots = 2
        cap0 = total // 4 + 4096
        assembled = None
        if rank == 0:
            assembled = [D.Assembled(torch.empty(8 * plan.n_windows, dtype=torch.int32, device=dev),
                                     torch.empty(4 * plan.n_tiles, dtype=torch.int32, device=dev),
                                     torch.empty(cap0, dtype=torch.int32, device=dev), 0, [0] * world) for _ in range(slots)]
        shard = D.HipShard(plan, rank, dev, slots=slots, assembled=assembled)
        in_ptr = buf.data_ptr()
        pending = [None] * slots
        n_local = [0] * slots
        dir_only = [False]

        def step(i):
            j = i % slots
            if pending[j] is not None:
                pending[j].wait()
                pending[j] = None
            shard.scan(in_ptr, sptr, j)
            n_local[j] = shard.finish(in_ptr, sptr, j)
            pending[j] = D.gather_shards(plan, rank, shard.windows[j], shard.stats[j], shard.dense[j], n_local[j], dst=0,
                                         out=assembled[j] if rank == 0 else None, async_op=True, directory_only=dir_only[0])

        def drain():
            for j in range(slots):
                if pending[j] is not None:
                    pending[j].wait()
                    pending[j] = None

        settle(step, drain)
        for i in range(max(args.warmup, slots)):
            step(i)
        drain()
        for j in range(slots):                                   # (a sync also grows a shard's match regions if they overflowed)
            shard.kernel_ms(j)
        tmax, dev_ms = timed(step, drain, args.steps)
        last = (args.steps - 1) % slots
        km = [shard.kernel_ms(j) for j in range(slots)]
        launches = sum(k[1] for k in km)
        kern_ms = sum(k[0] * k[1] for k in km) / max(1, launches)
        rinfo = km[last][2]
        alg_bytes = int(rinfo.algorithmic_bytes)

        # the summaries-only variant, measured not argued: only the tile directory (16 B per tile) travels
        dir_only[0] = True
        t_dir, _ = timed(step, drain, args.steps)
        dir_only[0] = False
        # where a step's time goes when nothing overlaps: scan + export / exchange / merge, each waited for
        nb = min(10, args.steps)
        t_scan = t_x = t_merge = 0.0
        for i in range(nb):
            barrier()
            c0 = time.perf_counter()
            shard.scan(in_ptr, sptr, 0)
            nl = shard.finish(in_ptr, sptr, 0)
            torch.cuda.synchronize()
            c1 = time.perf_counter()
            a = D.gather_shards(plan, rank, shard.windows[0], shard.stats[0], shard.dense[0], nl, dst=0,
                                out=assembled[0] if rank == 0 else None)
            torch.cuda.synchronize()
            c2 = time.perf_counter()
            if rank == 0:
                hb = D.adopt(plan, a, sptr)
                L.ts_batch_destroy(hb)
            c3 = time.perf_counter()
            t_scan += c1 - c0; t_x += c2 - c1; t_merge += c3 - c2
        split = {"scan_export_ms": round(max_over_ranks(t_scan / nb) * 1e3, 4), "exchange_ms": round(max_over_ranks(t_x / nb) * 1e3, 4),
                 "merge_ms_rank0": round(t_merge / nb * 1e3, 4), "steps": nb,
                 "note": "serialised (each phase waited for on the host); the timed region overlaps the exchange of step i "
                         "with the scan of step i+1"}
        step(0)
        drain()
        a = assembled[0] if rank == 0 else None
        result_batch = D.adopt(plan, a, sptr) if rank == 0 else None
        n_matches = a.n_records if rank == 0 else 0
        n_windows, n_tiles = plan.n_windows, plan.n_tiles
        gather_bytes = (8 * 4 * plan.n_windows + 16 * plan.n_tiles + 4 * n_matches) if rank == 0 else 0
        own = plan.ranges[0]
        gather_bytes_rx = gather_bytes - (32 * (own.window_end - own.window_begin) + 16 * (own.tile_end - own.tile_begin)
                                          + 4 * (a.counts[0] if rank == 0 else 0)) if rank == 0 else 0
        if plan.wire16_ok:
            gather_bytes_rx //= 2                               # every value travels as u16 and is widened on rank 0
        extra_cfg = {"timed_region": "resident ASCII in HBM on %d ranks (consecutive tile ranges of ONE plan) -> scan + tile-ordered "
                                     "export + ONE exchange (all-gather of record counts, grouped send/recv of window records, tile "
                                     "directory, match records) -> the whole assembly's results in rank 0's HBM; exchange of step i "
                                     "overlaps scan of step i+1" % world,
                     "backend": backend + ("" if backend == "nccl" else " (rehearsal: ranks share a GPU, tensors staged through the host)"),
                     "bases_per_rank": [int(x.bases) for x in plan.ranges],
                     "records_per_rank": a.counts if rank == 0 else None,
                     "gather_bytes_per_step": {"assembled_on_rank0": gather_bytes, "received_over_links": gather_bytes_rx,
                                               "wire_format": "u16 per value (records, tile counts and window fields all fit), widened on rank 0"
                                                              if plan.wire16_ok else "u32"},
                     "step_split": split,
                     "summaries_only_variant": {"ms_per_step": round(t_dir / args.steps * 1e3, 4),
                                                "value": round(total / (t_dir / args.steps) / 1e9, 3),
                                                "what_travels": "tile directory entries only (16 B per tile: %d B per step)" % (16 * plan.n_tiles)}}
        bases_done = total

    if rank == 0:
        ms_per_step = tmax / args.steps * 1e3
        value = bases_done / (tmax / args.steps) / 1e9
        achieved = alg_bytes / (kern_ms * 1e-3) / 1e9
        traffic, traffic_source = traffic_from_profile(args) if world == 1 else (None, None)
        out = {
            "metric": "Gbases/s scanned (whole node), 3 Gb FASTA TTAGGG w=1000 s=500",
            "value": round(value, 3), "unit": "Gbases/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
            "scaling": "weak" if (world > 1 and args.weak) else "strong", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": "%s: synthetic %.2f Gb / %d contigs%s, %s, %d patterns k=%d"
                                   % (("configs[1]" if world == 1 else "configs[2]") if args.flags == FLAGS and args.gbases == 3.0 else "custom",
                                      args.gbases, n, " per GPU" if args.weak and world > 1 else (" sharded over %d GPUs" % world if world > 1 else ""),
                                      args.flags, len(ui.patternInfo), len(ui.patternInfo[0][0])),
                       "bases": total, "windows": n_windows, "matches": n_matches, "tiles": n_tiles,
                       "device_ms_per_step_events": round(dev_ms, 4),
                       "host_enqueue_ms_per_step": round(enqueue_s[0] / max(1, args.steps) * 1e3, 4),
                       "settle": "%d untimed scans before the %d warm-up steps: the device's launch time needs ~40 launches to reach "
                                 "its steady state (profiles/r02/launch_ramp.txt)" % (settle_info["launches"], args.warmup), **extra_cfg},
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                         "traffic_source": traffic_source,
                         "kernel": "ts_scan_tiles" + (" (rank 0's range)" if strong else ""), "kernel_ms": round(kern_ms, 4),
                         "launches_timed": launches, "algorithmic_bytes": alg_bytes},
        }
        if world == 1 and args.full and not os.environ.get("TS_BENCH_NO_BOX_PROBE"):
            # what THIS box issues and streams (ts_box_probe: hand-written independent integer instructions at four waves per SIMD;
            # a 1 GiB copy), measured right after the timed steps, for context: the boxes of this pool differ by up to 7 % on one
            # kernel hash (0.705 .. 0.758 ms per step).  The short probes do not explain that spread (0.720 / 0.727 / 0.739 / 0.758 ms
            # at 580 / 567 / 585 / 583 wave-instructions per ns): they say what a plain copy moves on the box — 4.65-4.78 TB/s
            vi, cb = C.c_double(0), C.c_double(0)
            if L.ts_box_probe(tel._ctx.ptr, C.byref(vi), C.byref(cb)) == 0:
                out["roofline"]["box"] = {"valu_wave_instr_per_ns": round(vi.value, 1), "copy_read_plus_write_gbs": round(cb.value, 1),
                                          "note": "device-wide issue rate of independent v_and_b32 at 4 waves per SIMD; 16-byte grid-strided copy of 1 GiB"}
                # spread or regression?  this box's kernel time over the fastest box the SAME kernel source has met (kept beside
                # the PMC traffic, under the same hash): 1.00-1.10 is the pool's spread, more than that is not
                fast = fastest_box_seen(args)
                if fast:
                    out["roofline"]["box"]["kernel_ms_over_fastest_box_seen"] = round(kern_ms / fast, 3)
                    out["roofline"]["box"]["fastest_box_seen_kernel_ms"] = fast
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args, opts, buf, offsets, lens)
        if args.verify and sharded is not None:
            # shard results: a single-GPU scan of the whole assembly on rank 0 is (a) checked against the independent torch
            # computation and (b) compared, segment by segment, with what the ranks' messages merged to
            one = D.ShardPlan(tel, lens, world=1)
            if L.ts_batch_scan(one.batch, C.c_void_p(full.data_ptr()), sptr) != 0 or L.ts_batch_sync(one.batch) != 0:
                raise RuntimeError(tel._ctx.error())
            out["verify"] = verify_full_size(L, one.batch, tel, full, offsets, lens, ui, dev)
            out["verify"]["sharded_equals_single_gpu"] = compare_sharded_with_single_gpu(L, K, tel, one.batch, sharded, n, n_matches <= 600_000_000)   # (16 B per match record on the host: 1.5 GB at configs[1], 0.7 GB at configs[4])
            one.close()
        elif args.verify:
            out["verify"] = verify_full_size(L, result_batch, tel, full if strong else buf, offsets, lens, ui, dev)
            if strong:
                # the assembled arrays against a single-GPU scan of the whole assembly, bit for bit
                one = D.ShardPlan(tel, lens, world=1)
                hs = D.HipShard(one, 0, dev, slots=1)
                hs.scan(full.data_ptr(), sptr, 0)
                n1 = hs.finish(full.data_ptr(), sptr, 0)
                a = assembled[0]
                assert n1 == a.n_records, (n1, a.n_records)
                assert torch.equal(hs.windows[0], a.windows) and torch.equal(hs.stats[0], a.stats)
                assert torch.equal(hs.dense[0][:n1], a.dense[:n1])
                out["verify"]["sharded_equals_single_gpu"] = {"windows": int(plan.n_windows), "tiles": int(plan.n_tiles), "records": int(n1)}
                hs.close()
        if args.blocks:
            seg_out = (K.SegmentOut * n)()
            b0 = time.perf_counter()
            rc = L.ts_batch_download_blocks(result_batch, seg_out)
            bdt = time.perf_counter() - b0
            if rc != 0:
                raise RuntimeError(tel._ctx.error())
            out["device_block_calling"] = {
                "wall_ms_incl_alloc_d2h_windows": round(bdt * 1e3, 2),
                "terminal_blocks": int(sum(seg_out[i].n_terminal_blocks for i in range(n))),
                "interstitial_blocks": int(sum(seg_out[i].n_interstitial_blocks for i in range(n)))}
            L.ts_free_segments(seg_out, n)
        if world == 1 and args.full and not forced_strong and not os.environ.get("TS_BENCH_NO_BLOCKS_RECORD"):
            out["scan_plus_block_calling"] = scan_plus_block_calling_record(args, tel, lens, buf, dev, out["ms_per_step"], stream)
        if world == 1 and args.full and not args.no_reads and not forced_strong:
            from .reads import reads_sub_record
            out["reads"] = reads_sub_record(args, dev)
        if world == 1 and args.full and not args.no_e2e:
            out["pcie_inclusive"] = pcie_inclusive(L, K, tel, buf, offsets, lens, total)
            out["pcie_inclusive"]["host_placement"] = ("process and library threads on NUMA node %d, the GPU's" % common.HOST_NUMA_NODE
                                                       if common.HOST_NUMA_NODE is not None else "not bound to a NUMA node")
        print(json.dumps(out), flush=True)
    if strong:
        if result_batch:
            L.ts_batch_destroy(result_batch)
        if sharded is not None:
            D.free_segments(plan, sharded["seg_out"])
        shard.close()
    barrier()


def scan_plus_block_calling_record(args, tel, lens, buf, dev, plain_ms, stream):
    """What a rank of the sharded job does per step, on this one GPU with the whole assembly: the EMITTING scan
    (ts_batch_set_emit: visible records + chain summaries) + block calling on the device + the packed message — the
    reference's scanSegment contains block calling (src/teloscope.cpp:642-657), the plain scan that `value` times does not.
    This is the like-for-like origin of a 1 -> N curve: the N > 1 lines time exactly this per rank, plus the exchange."""
    import torch
    import teloscope_amd.distributed as D
    steps, slots = min(args.steps, 40), max(2, int(os.environ.get("TS_BENCH_SLOTS", "4")))
    plan = D.ShardPlan(tel, lens, world=1)
    shard = D.PackedShard(plan, 0, dev, slots=slots, scale=1)
    shard.set_timing(0)                                       # (no kernel times are read from these steps)
    sptr = C.c_void_p(stream.cuda_stream)                     # (the stream the plain scans ran on: streams share a few hardware queues)
    pack_streams = D.concurrent_streams(tel, dev, 3, first=stream)[1:]      # (not on the scan stream's hardware queue)
    packed = [torch.cuda.Event() for _ in range(slots)]
    used = [False] * slots
    in_ptr = buf.data_ptr()

    def step(i):
        j = i % slots
        ps = pack_streams[j % 2]
        if used[j]:
            stream.wait_event(packed[j])
        shard.scan(in_ptr, sptr, j)
        with torch.cuda.stream(ps):
            shard.wait_scan(C.c_void_p(ps.cuda_stream), j)       # (the library's own event behind the scan)
            shard.pack(C.c_void_p(ps.cuda_stream), j)
            packed[j].record(ps)
        used[j] = True

    def settle_regions():
        for _ in range(6):
            for i in range(slots):
                step(i)
            torch.cuda.synchronize()
            st = [shard.status(j) for j in range(slots)]
            if any(x.flags & K_SHARD_SCAN for x in st):
                for j in range(slots):
                    shard.sync(j)
            elif any(x.flags & K_SHARD_GROW for x in st):
                shard.set_scale(shard.scale * 2)
            else:
                return st[0]
        raise RuntimeError("scan_plus_block_calling: the message kept overflowing")

    from teloscope_amd import _capi as K
    K_SHARD_SCAN, K_SHARD_GROW = K.SHARD_OVERFLOW_SCAN, K.SHARD_OVERFLOW_VISIBLE | K.SHARD_OVERFLOW_BLOCKS
    with torch.cuda.stream(stream):
        st0 = settle_regions()
        for i in range(3 * slots):
            step(i)
        torch.cuda.synchronize()
        c0 = time.perf_counter()
        for i in range(steps):
            step(i)
        torch.cuda.synchronize()
        overlapped = (time.perf_counter() - c0) / steps * 1e3
        # serialised: scan, then block calling + pack, each waited for
        t_scan = t_pack = 0.0
        nb = min(10, steps)
        for i in range(nb):
            c0 = time.perf_counter()
            shard.scan(in_ptr, sptr, 0)
            torch.cuda.synchronize()
            c1 = time.perf_counter()
            shard.pack(sptr, 0)
            torch.cuda.synchronize()
            t_scan += c1 - c0
            t_pack += time.perf_counter() - c1
    rec = {"ms_per_step": round(overlapped, 4), "gbases_per_s": round(sum(lens) / overlapped / 1e6, 1), "steps": steps,
           "emitting_scan_alone_ms": round(t_scan / nb * 1e3, 4), "block_calling_and_pack_alone_ms": round(t_pack / nb * 1e3, 4),
           "plain_scan_ms_per_step": round(plain_ms, 4),
           "blocks": int(st0.n_blocks), "visible_records": int(st0.n_visible), "message_bytes": int(shard.info.msg_bytes),
           "what": "emitting scan + terminal / interstitial block calling on the device + packed message (bit-packed windows, visible "
                   "records, blocks), %d buffer slots, pack beside the next scan; results stay in HBM" % slots}
    shard.close()
    plan.close()
    return rec
