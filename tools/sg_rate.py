#!/usr/bin/env python3
"""Scatter-gather checksum rate on the MI355X ("scatter-gather").

GPU only: fails without one. For each workload it times, in one process and
alternating burst by burst,

  (a) tulips_csum_batch_sg on the fragments where they lie,
  (b) what an integrator does without it: gather the fragments into a
      contiguous arena, then checksum that
        SPLIT1500  two strided device copies + tulips_csum_batch_fixed
                   (and, for comparison, the gather kernel below + the same)
        ZIPF-SG    one gather kernel (GATHER_SRC below, compiled here with
                   hipcc when the tool starts) + tulips_csum_batch,
  (c) the contiguous call alone on pre-gathered data.

Workloads
  SPLIT1500  65,536 TCP segments of 1500 B: fragment 0 a 20-byte header at
             hdr + 64*i, fragment 1 1480 B at pay + 1480*i.
  ZIPF-SG    the ZIPF lengths of BASELINE configs[3] (orc_zipf_lengths), each
             cut at seeded points into 1 to 4 fragments, the fragments placed
             in shuffled order at seeded byte alignments in one arena.

Method: seeded data (splitmix), at least four distinct batches per workload
and more than 256 MB of them so nothing is MALL-resident, a warm-up, then
>= 15 timed bursts of >= 20 launches between device events per variant
(each burst one captured graph, so no figure holds the host's enqueue cost).
Every burst's outputs are compared with the CPU oracle over the concatenated
bytes. Reported: per-launch median and range in microseconds.

The one bar: (a) faster than (b) on both workloads (exit status 1 if not).
(a)/(c), the price of fragment metadata and extra edge chunks, is recorded
without a bar. Writes one JSON document (--out).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# The integrator's gather: one wave per fragment; a lane writes one aligned
# destination dword made of the two aligned source dwords that hold its bytes
# (any relative alignment), the partial first and last dwords byte by byte.
# Source dword loads stay inside the 4-byte-aligned hull of the fragment.
GATHER_SRC = r"""
#include <hip/hip_runtime.h>
#include <stdint.h>
extern "C" __global__ __launch_bounds__(256) void
sg_gather(const uint8_t* __restrict__ base, const uint64_t* __restrict__ foffs,
          const uint16_t* __restrict__ flens, const uint64_t* __restrict__ doffs,
          uint8_t* __restrict__ dest, uint32_t nfrags)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t j = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (j >= nfrags) {
    return;
  }
  const uint32_t len = flens[j];
  const uint8_t* s = base + foffs[j];
  uint8_t* d = dest + doffs[j];
  // [d, d + len) = head bytes up to the first aligned dword, body, tail bytes
  const uint32_t head = min(len, uint32_t((4 - (reinterpret_cast<uintptr_t>(d) & 3)) & 3));
  const uint32_t words = (len - head) >> 2;
  const uint32_t tail0 = head + 4 * words;
  if (lane < head) {
    d[lane] = s[lane];
  }
  if (lane >= 32 && lane - 32 < len - tail0) {
    d[tail0 + lane - 32] = s[tail0 + lane - 32];
  }
  const uint8_t* sb = s + head;
  const uint32_t sh = 8 * uint32_t(reinterpret_cast<uintptr_t>(sb) & 3);
  const uint32_t* sw = reinterpret_cast<const uint32_t*>(reinterpret_cast<uintptr_t>(sb) & ~uintptr_t(3));
  uint32_t* dw = reinterpret_cast<uint32_t*>(d + head);
  for (uint32_t w = lane; w < words; w += 64) {
    const uint32_t lo = sw[w];
    const uint32_t hi = sh ? sw[w + 1] : 0u;
    dw[w] = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
  }
}

extern "C" int
sg_gather_launch(const void* base, const void* foffs, const void* flens, const void* doffs,
                 void* dest, uint32_t nfrags, void* stream)
{
  if (nfrags == 0) {
    return 0;
  }
  hipLaunchKernelGGL(sg_gather, dim3((nfrags + 3) / 4), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const uint8_t*>(base),
                     static_cast<const uint64_t*>(foffs), static_cast<const uint16_t*>(flens),
                     static_cast<const uint64_t*>(doffs), static_cast<uint8_t*>(dest), nfrags);
  return int(hipGetLastError());
}
"""

N = 65536
HDR, PAY, SEG = 20, 1480, 1500
HDR_STRIDE = 64


def build_gather(workdir):
    """Compile GATHER_SRC for gfx950 and load it (after torch, so that it binds
    the HIP runtime already in the process)."""
    src = os.path.join(workdir, "sg_gather.hip")
    lib = os.path.join(workdir, "libsg_gather.so")
    with open(src, "w") as f:
        f.write(GATHER_SRC)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                    "-o", lib, src], check=True)
    L = C.CDLL(lib)
    L.sg_gather_launch.restype = C.c_int
    L.sg_gather_launch.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
    return L


def zipf_sg_plan(orc, seed, n=N):
    """ZIPF-SG: (frag_offsets, frag_lengths, seg_first, gathered offsets of
    the fragments, segment lengths, arena bytes)."""
    rng = np.random.default_rng(seed)
    lens = orc.zipf_lengths(n).astype(np.int64)
    k = np.minimum(rng.integers(1, 5, n), np.maximum(lens, 1))       # fragments per segment
    first = np.concatenate(([0], np.cumsum(k)))
    nf = int(first[-1])
    seg_of = np.repeat(np.arange(n), k)
    # seeded cut points inside each segment, sorted per segment
    cuts = rng.integers(0, np.repeat(lens, k) + 1)
    cuts[first[:-1]] = 0
    order = np.lexsort((cuts, seg_of))
    cuts = cuts[order]
    ends = np.concatenate((cuts[1:], [0]))
    ends[first[1:] - 1] = lens                                       # last fragment ends the segment
    flens = ends - cuts
    assert (flens >= 0).all() and int(flens.sum()) == int(lens.sum())
    seg_start = np.concatenate(([0], np.cumsum(lens)))[:-1]
    doffs = seg_start[seg_of] + cuts                                 # where a gather puts each fragment
    # shuffled placement at seeded byte alignments
    place = rng.permutation(nf)
    gap = rng.integers(0, 16, nf)
    pos = np.zeros(nf, dtype=np.int64)
    pos[place] = np.cumsum(flens[place] + gap[place]) - flens[place]
    nbytes = int(pos.max(initial=0) + flens.max(initial=0)) + 64
    return (pos.astype(np.uint64), flens.astype(np.uint16), first.astype(np.uint32),
            doffs.astype(np.uint64), lens.astype(np.uint16), nbytes)


def stats(us):
    us = np.sort(np.asarray(us))
    return {"median_us": round(float(np.median(us)), 3), "min_us": round(float(us[0]), 3),
            "max_us": round(float(us[-1]), 3), "bursts": len(us)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sg_rate.json"))
    ap.add_argument("--bursts", type=int, default=15)
    ap.add_argument("--launches", type=int, default=24)
    args = ap.parse_args()
    if args.bursts < 15 or args.launches < 20:
        ap.error("at least 15 bursts of at least 20 launches")

    from oracle import MODE_RAW, MODE_TCP, Oracle, packed_offsets
    orc = Oracle()
    zplan = zipf_sg_plan(orc, 0x5A53)          # host work first: a rehearsal gets this far

    import torch
    if not torch.cuda.is_available():
        sys.exit("sg_rate: needs an MI355X (no GPU found)")
    import benchlib
    from tulips_amd import csum
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    tmp = tempfile.TemporaryDirectory()
    gather = build_gather(tmp.name)

    def d(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def fill(nbytes, byte_off):
        t = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
        benchlib.fill_splitmix(t, nbytes, byte_off=byte_off)
        t[nbytes:].zero_()
        return t

    graphs = []      # kept to the end of the process

    def time_variants(variants, check):
        """variants: name -> launch(batch index, stream). Each variant's burst
        (its launches rotating through the batches) is captured once into a
        HIP graph, so that the host's enqueue cost is in no figure; bursts of
        the variants alternate, and every burst's outputs are checked.
        Returns name -> stats."""
        burst = {}
        for name, fn in variants.items():
            for b in range(nbatch[0]):                 # warm-up: every batch once
                fn(b, torch.cuda.current_stream().cuda_stream)
            check(name)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                cs = torch.cuda.current_stream().cuda_stream
                for i in range(args.launches):
                    fn(i % nbatch[0], cs)
            graphs.append(g)
            clear()
            g.replay()
            check(name)
            burst[name] = g
        t = {name: [] for name in variants}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.bursts):
            for name, g in burst.items():
                clear()
                e0.record()
                g.replay()
                e1.record()
                e1.synchronize()
                t[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)
                check(name)
        return {name: stats(v) for name, v in t.items()}

    nbatch = [0]
    result = {"tool": "tools/sg_rate.py", "device": torch.cuda.get_device_name(0),
              "library": csum.version(), "segments": N, "bursts": args.bursts,
              "launches_per_burst": args.launches, "unit": "microseconds per launch",
              "workloads": {}}

    def sweep(run_a, check):
        out = {}
        for s, u in csum.SG_GEOMETRIES:
            tn = csum.Tuning(kind=csum.KIND_DEFAULT, group=s, unroll=u)
            out[f"{s}x{u}"] = time_variants({"a": lambda b, sp, tn=tn: run_a(b, sp, tn)}, check)["a"]
        return out

    # ---- SPLIT1500 ---------------------------------------------------------
    nb = 4
    nbatch[0] = nb
    hdr_bytes, pay_bytes = HDR_STRIDE * N, PAY * N
    i64 = np.arange(N, dtype=np.uint64)
    foffs = np.empty(2 * N, dtype=np.uint64)
    foffs[0::2] = HDR_STRIDE * i64
    foffs[1::2] = hdr_bytes + PAY * i64
    flens = np.tile(np.array([HDR, PAY], dtype=np.uint16), N)
    first = (2 * np.arange(N + 1)).astype(np.uint32)
    doffs = np.empty(2 * N, dtype=np.uint64)
    doffs[0::2] = SEG * i64
    doffs[1::2] = SEG * i64 + HDR
    rng = np.random.default_rng(1500)
    src = rng.integers(0, 2**32, N, dtype=np.uint64).astype(np.uint32)
    dst = rng.integers(0, 2**32, N, dtype=np.uint64).astype(np.uint32)
    dfo, dfl, dfi, ddo, dsrc, ddst = d(foffs), d(flens), d(first), d(doffs), d(src), d(dst)
    arenas, packed, expect = [], [], []
    for b in range(nb):
        a = fill(hdr_bytes + pay_bytes, byte_off=b * (hdr_bytes + pay_bytes))
        h = a.cpu().numpy()
        flat = np.concatenate((h[:hdr_bytes].reshape(N, HDR_STRIDE)[:, :HDR],
                               h[hdr_bytes:hdr_bytes + pay_bytes].reshape(N, PAY)), axis=1)
        flat = np.ascontiguousarray(flat).reshape(-1)
        expect.append(d(orc.batch(flat, stride=SEG, fixed_len=SEG, n=N, src=src, dst=dst,
                                  mode=MODE_TCP, nthreads=8).view(np.int16)))
        arenas.append(a)
        packed.append(d(np.concatenate((flat, np.zeros(64, np.uint8)))))
        del h, flat
    scratch = torch.zeros(SEG * N + 64, dtype=torch.uint8, device=dev)
    outs = [torch.zeros(N, dtype=torch.int16, device=dev) for _ in range(nb)]

    def clear():
        for o in outs:
            o.zero_()

    def check(name):
        torch.cuda.synchronize()
        for b in range(nbatch[0]):
            if not torch.equal(outs[b], expect[b]):
                raise SystemExit(f"sg_rate: {name} batch {b} differs from the oracle")

    s32 = scratch[:SEG * N].view(torch.int32).view(N, SEG // 4)

    def split_a(b, sp, tn=None):
        csum.batch_sg(arenas[b], dfo, dfl, dfi, src=dsrc, dst=ddst, mode=MODE_TCP, out=outs[b],
                      stream=sp, tuning=tn)

    def split_b(b, sp):
        a32 = arenas[b][:hdr_bytes + pay_bytes].view(torch.int32)
        s32[:, :HDR // 4].copy_(a32[:hdr_bytes // 4].view(N, HDR_STRIDE // 4)[:, :HDR // 4])
        s32[:, HDR // 4:].copy_(a32[hdr_bytes // 4:].view(N, PAY // 4))
        csum.batch_fixed(scratch, SEG, SEG, N, src=dsrc, dst=ddst, mode=MODE_TCP, out=outs[b],
                         stream=sp)

    def split_b_kernel(b, sp):
        rc = gather.sg_gather_launch(arenas[b].data_ptr(), dfo.data_ptr(), dfl.data_ptr(),
                                     ddo.data_ptr(), scratch.data_ptr(), 2 * N, sp)
        assert rc == 0, rc
        csum.batch_fixed(scratch, SEG, SEG, N, src=dsrc, dst=ddst, mode=MODE_TCP, out=outs[b],
                         stream=sp)

    def split_c(b, sp):
        csum.batch_fixed(packed[b], SEG, SEG, N, src=dsrc, dst=ddst, mode=MODE_TCP, out=outs[b],
                         stream=sp)

    r = time_variants({"a_batch_sg": split_a, "b_copies_then_batch_fixed": split_b,
                       "b_gather_kernel_then_batch_fixed": split_b_kernel,
                       "c_batch_fixed_pregathered": split_c}, check)
    r["instances_a"] = sweep(split_a, check)
    r["bytes_per_batch"] = SEG * N
    r["batches"] = nb
    r["fragments"] = 2 * N
    result["workloads"]["SPLIT1500"] = r
    del arenas, packed, expect, scratch, s32, outs
    torch.cuda.empty_cache()

    # ---- ZIPF-SG -----------------------------------------------------------
    zfo, zfl, zfi, zdo, zlens, znbytes = zplan
    zbytes = int(zlens.astype(np.int64).sum())
    nb = max(4, -(-(280 << 20) // max(zbytes, 1)))
    nbatch[0] = nb
    zoffs = packed_offsets(zlens)
    dfo, dfl, dfi, ddo = d(zfo), d(zfl), d(zfi), d(zdo)
    dzo, dzl = d(zoffs), d(zlens)
    nf = len(zfo)
    arenas, packed, expect = [], [], []
    fo64, fl64, do64 = zfo.astype(np.int64), zfl.astype(np.int64), zdo.astype(np.int64)
    # gather index on the host (the oracle's concatenated bytes)
    fpos = np.concatenate(([0], np.cumsum(fl64)))
    idx = np.repeat(fo64 - do64, fl64)           # source - destination, per byte
    dpos = np.repeat(do64, fl64) + (np.arange(int(fpos[-1])) - np.repeat(fpos[:-1], fl64))
    for b in range(nb):
        a = fill(znbytes, byte_off=b * znbytes)
        h = a.cpu().numpy()
        flat = np.zeros(zbytes + 64, dtype=np.uint8)
        flat[dpos] = h[dpos + idx]
        expect.append(d(orc.batch(flat, zoffs, zlens, mode=MODE_RAW, nthreads=8).view(np.int16)))
        arenas.append(a)
        packed.append(d(flat))
        del h, flat
    del idx, dpos
    scratch = torch.zeros(zbytes + 64, dtype=torch.uint8, device=dev)
    outs = [torch.zeros(N, dtype=torch.int16, device=dev) for _ in range(nb)]

    def zipf_a(b, sp, tn=None):
        csum.batch_sg(arenas[b], dfo, dfl, dfi, mode=MODE_RAW, out=outs[b], stream=sp, tuning=tn)

    def zipf_b(b, sp):
        rc = gather.sg_gather_launch(arenas[b].data_ptr(), dfo.data_ptr(), dfl.data_ptr(),
                                     ddo.data_ptr(), scratch.data_ptr(), nf, sp)
        assert rc == 0, rc
        csum.batch(scratch, dzo, dzl, mode=MODE_RAW, out=outs[b], stream=sp)

    def zipf_c(b, sp):
        csum.batch(packed[b], dzo, dzl, mode=MODE_RAW, out=outs[b], stream=sp)

    r = time_variants({"a_batch_sg": zipf_a, "b_gather_kernel_then_batch": zipf_b,
                       "c_batch_pregathered": zipf_c}, check)
    r["instances_a"] = sweep(zipf_a, check)
    r["bytes_per_batch"] = zbytes
    r["batches"] = nb
    r["fragments"] = nf
    result["workloads"]["ZIPF-SG"] = r

    ok = True
    for name, w in result["workloads"].items():
        a = w["a_batch_sg"]["median_us"]
        bs = [v["median_us"] for k, v in w.items() if k.startswith("b_")]
        c = [v["median_us"] for k, v in w.items() if k.startswith("c_")][0]
        w["a_over_best_b"] = round(a / min(bs), 3)
        w["a_over_c"] = round(a / c, 3)
        w["a_gbytes_per_s"] = round(w["bytes_per_batch"] / a / 1e3, 1)
        w["a_beats_b"] = a < min(bs)
        ok = ok and w["a_beats_b"]
    result["bar_a_beats_b_on_both"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    torch.cuda.synchronize()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
