#!/usr/bin/env python3
"""What the datagram wire format costs on the GPU: noise_gpu_dgram_open against
noise_gpu_cswin_decrypt_records, and noise_gpu_dgram_seal against
noise_gpu_cs_encrypt_records, each control running on descriptors built
beforehand (the host walk that the datagram calls remove is left out of the
timing, so the difference is what parse / build / finish cost on the device).
One box, one run, the variants alternating call by call; noise_gpu_cs_assign
alone is timed in the same loop as the yardstick.  Shape: 64 Ki sessions x 16
packets at 1 KiB and at 64-byte payloads, packet slots at 16-byte aligned
addresses (stride 32 + len), the wire order shuffled inside every session;
every timed open starts from fresh windows (a reset, timed alone as well), so
that every packet is decrypted and accepted.  Device-resident, HIP-event timed;
GiB/s of payload.
    python tools/bench_dgram.py [--out profiles/dgram/bench.json]
                                [--sessions N] [--per-session N] [--lens L ...] [--iters K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "noise-cpp_amd", "python"))
import noise_amd  # noqa: E402

TYPE = 4


def timed(torch, fns, iters):
    """Mean milliseconds per call of each fn, the fns alternating inside every iteration."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)]
    ms = [0.0] * len(fns)
    for _ in range(iters):
        ev[0].record()
        for k, fn in enumerate(fns):
            fn()
            ev[k + 1].record()
        torch.cuda.synchronize()
        for k in range(len(fns)):
            ms[k] += ev[k].elapsed_time(ev[k + 1])
    return [m / iters for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dgram", "bench.json"))
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--per-session", type=int, default=16)
    ap.add_argument("--lens", type=int, nargs="+", default=[1024, 64])
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    import torch
    noise_amd.load()
    torch.cuda.set_device(0)
    S, P = a.sessions, a.per_session
    R = S * P
    d_keys = torch.empty(S * 32, dtype=torch.uint8, device="cuda")
    noise_amd.fill_synthetic(d_keys, S * 32, 0x4B4559)
    i = torch.arange(R, dtype=torch.int64, device="cuda")
    d_idx = (i % S).to(torch.int32)  # interleaved: consecutive packets belong to different sessions
    # the wire: packet k of a session carries a counter drawn from a permutation of its P counters
    gen = torch.Generator(device="cuda").manual_seed(1)
    perm = torch.rand(S, P, device="cuda", generator=gen).argsort(dim=1)
    src = (perm.t().contiguous() * S + torch.arange(S, device="cuda")).reshape(-1)  # wire slot -> sealed packet
    tx, txc, rx, rxc = (noise_amd.CipherStateTable(S) for _ in range(4))
    d_scr = torch.empty(R, dtype=torch.int64, device="cuda")
    d_ast = torch.empty(R, dtype=torch.uint8, device="cuda")
    rows = []
    for L in a.lens:
        C = L + 32
        d_pt = torch.empty(R * L, dtype=torch.uint8, device="cuda")
        noise_amd.fill_synthetic(d_pt, R * L, 7)
        d_pkt, d_pktc, d_back = (torch.empty(n, dtype=torch.uint8, device="cuda") for n in (R * C, R * C, R * L))
        d_recs, d_wrecs = (torch.empty(R * 48, dtype=torch.uint8, device="cuda") for _ in range(2))
        d_st, d_stc = (torch.empty(R, dtype=torch.uint8, device="cuda") for _ in range(2))
        d_len = torch.empty(R, dtype=torch.int32, device="cuda")
        for t in (tx, txc, rx, rxc):
            t.set(0, S, d_keys)  # counters back to 0, fresh windows
        pay, slots = noise_amd.span(d_pt, stride=L, length=L), noise_amd.span(d_pkt, stride=C)

        def seal():
            tx.seal_datagrams(TYPE, d_idx, pay, slots, d_recs, d_st, R, d_pkt_len=d_len, len_sum=R * L)

        # ---- the first seal is the control's batch: same counters, same bytes
        seal()
        d_crecs = d_recs.clone()  # descriptors built beforehand: in_off, out_off, len, key_idx

        def seal_ctl():
            txc.encrypt_records(d_crecs, R, d_pt, d_pktc, d_status=d_stc, len_sum=R * L)

        seal_ctl()
        torch.cuda.synchronize()
        pk, pkc = d_pkt.view(R, C), d_pktc.view(R, C)
        assert int(d_st.sum()) == 0 and int(d_stc.sum()) == 0 and bool((d_len == C).all())
        assert torch.equal(pk[:, 16:], pkc[:, 16:])
        hdr = pk[:, :16].contiguous()
        assert torch.equal(hdr.view(torch.int32)[:, 0], torch.full((R,), TYPE, dtype=torch.int32, device="cuda"))
        assert torch.equal(hdr.view(torch.int32)[:, 1], d_idx) and torch.equal(hdr.view(torch.int64)[:, 1], i // S)
        d_wire = pk[src].contiguous().reshape(-1)  # shuffled inside every session
        want = d_pt.view(R, L)[src].reshape(-1)
        wire, back = noise_amd.span(d_wire, stride=C, length=C), noise_amd.span(d_back, stride=L)

        def open_():
            rx.window_reset(0, S)
            rx.open_datagrams(TYPE, wire, back, d_wrecs, d_st, R, d_payload_len=d_len, len_sum=R * L)

        d_back.zero_()
        open_()
        torch.cuda.synchronize()
        assert int(d_st.sum()) == 0 and torch.equal(d_back, want) and bool((d_len == L).all())
        d_cwrecs = d_wrecs.clone()  # what the host walk over the headers would have uploaded

        def open_ctl():
            rxc.window_reset(0, S)
            rxc.decrypt_records_window(d_cwrecs, R, d_wire, d_back, d_stc, len_sum=R * L)

        def reset():
            rxc.window_reset(0, S)

        def assign():
            txc.assign(d_idx, d_scr, R, d_ast)

        d_back.zero_()
        open_ctl()
        torch.cuda.synchronize()
        assert int(d_stc.sum()) == 0 and torch.equal(d_back, want)
        fns = [seal, seal_ctl, assign, open_, open_ctl, reset]
        for _ in range(3):
            for fn in fns:
                fn()
        se, sc, am, op, oc, rs = timed(torch, fns, a.iters)
        torch.cuda.synchronize()
        assert int(d_st.sum()) == 0 and int(d_stc.sum()) == 0 and int(d_ast.sum()) == 0
        assert torch.equal(d_back, want)
        gib = R * L / 2.0 ** 30
        row = {"len": L, "packets": R, "sessions": S, "order": "shuffled inside each session",
               "seal_us": round(se * 1e3, 1), "cs_encrypt_records_us": round(sc * 1e3, 1),
               "seal_extra_us": round((se - sc) * 1e3, 1), "seal_GiBps": round(gib / (se / 1e3), 1),
               "open_us": round(op * 1e3, 1), "cswin_decrypt_records_us": round(oc * 1e3, 1),
               "open_extra_us": round((op - oc) * 1e3, 1), "open_GiBps": round(gib / (op / 1e3), 1),
               "assign_us": round(am * 1e3, 1), "window_reset_us": round(rs * 1e3, 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    for t in (tx, txc, rx, rxc):
        t.close()
    out = {"tool": "tools/bench_dgram.py", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "timing": "HIP events, variants alternating in one run; open and its control include a window reset",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
