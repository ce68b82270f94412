#!/usr/bin/env python3
"""K1 time of the decoded parse (TCBEE_F_DECODE) beside the default parse, in one
process, alternating rounds (tcbee_ctx_profile): config-3 style standard frames in
both modes, then decoded-only mixes built on the host from the synthetic trace —
every frame single-tagged, 10 % of the frames IHL 6 (general path), and IPv6 with
one hop-by-hop header. Prints one JSON line.

  python tools/decode_ab.py [--frames N] [--rounds R] [--iters I]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STRIDE = 128  # the host-built mixes keep the first 128 B of each frame (as the pipe's window)


def spliced(hdr, ln, at, blob, every=1, patch=()):
    """Frames `hdr` [n, 128] with `blob` inserted at byte `at` of every `every`-th frame
    and (byte, value) patches applied to those frames; caplens grow accordingly."""
    out, ln = hdr.copy(), ln.copy()
    sel = np.arange(0, len(hdr), every)
    out[sel, at + len(blob):] = hdr[sel, at:STRIDE - len(blob)]
    out[sel, at:at + len(blob)] = np.frombuffer(blob, np.uint8)
    for b, v in patch:
        out[sel, b] = v
    ln[sel] += len(blob)
    return out, ln


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    import torch
    import tcbee_amd
    n = args.frames
    torch.cuda.set_device(0)
    torch.cuda.set_stream(torch.cuda.Stream())
    stream = torch.cuda.current_stream().cuda_stream
    off, ln, ts, alen = tcbee_amd.synth_index(n, sizes="imix6")
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_len = torch.from_numpy(ln.view(np.int32)).cuda()
    d_ts = torch.from_numpy(ts.view(np.int64)).cuda()
    hdrs = {}
    for name, kind in (("v4", 1), ("v6", 3)):
        d_arena = torch.zeros(alen + STRIDE, dtype=torch.uint8, device="cuda")
        tcbee_amd.gen_frames_device(d_arena, d_off, d_len, n, kind, 10_000, 0x7CBEE, stream=stream)
        torch.cuda.synchronize()
        if name == "v4":
            std = d_arena
        idx = torch.from_numpy(off.astype(np.int64)).cuda()[:, None] + torch.arange(STRIDE, device="cuda")
        hdrs[name] = d_arena[idx].cpu().numpy()
    tag = b"\x81\x00\x00\x64"
    mixes = {"tagged": spliced(hdrs["v4"], ln, 12, tag),
             "general10": spliced(hdrs["v4"], ln, 34, b"\x01\x01\x01\x01", every=10, patch=((14, 0x46),)),
             "v6_hopbyhop": spliced(hdrs["v6"], ln, 54, b"\x06\x00" + bytes(6), patch=((20, 0),))}
    soff = torch.arange(n, dtype=torch.int64, device="cuda") * STRIDE
    work = {"standard": (std, alen, d_off, d_len)}
    for k, (h, l) in mixes.items():
        work[k] = (torch.from_numpy(h.reshape(-1)).cuda(), n * STRIDE, soff,
                   torch.from_numpy(l.view(np.int32)).cuda())
    d_rec = torch.empty(n * 74 + 64, dtype=torch.uint8, device="cuda")
    d_hash = torch.empty(n, dtype=torch.int32, device="cuda")
    d_id = torch.empty(n, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    res = {"frames": n, "rounds": args.rounds, "iters": args.iters}
    with tcbee_amd.PacketParser(max_frames=n, max_flows=1 << 16) as p:
        def k1_us(w, decode):
            a, al, o, l = work[w]
            p.reset_flows()
            p.profile(True)
            for _ in range(args.iters):
                p.parse_device(a, al, o, l, d_ts, n, d_rec, n, d_hash, d_id, d_n, d_ctr,
                               stream=stream, decode=decode)
            torch.cuda.synchronize()
            ms, k = p.profile_read()
            p.profile(False)
            return 1e3 * ms / k, int(d_n.item())
        runs = [("standard", False), ("standard", True)] + [(k, True) for k in mixes]
        for w, dec in runs:
            k1_us(w, dec)  # warm-up
        for w, dec in runs * args.rounds:  # alternating rounds
            us, recs = k1_us(w, dec)
            e = res.setdefault(f"{w}_{'decode' if dec else 'default'}", {"k1_us": [], "records": recs})
            e["k1_us"].append(round(us, 2))
        for e in res.values():
            if isinstance(e, dict):
                e["k1_ns_per_frame_median"] = round(1e3 * float(np.median(e["k1_us"])) / n, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
