#!/usr/bin/env python3
"""What length-prefixed stream framing costs on the GPU: noise_gpu_framed_seal
against noise_gpu_cs_encrypt_records, and noise_gpu_framed_open against
noise_gpu_cs_decrypt_records, each control running on descriptors built
beforehand of the identical unaligned layout (the host walk that the framing
calls remove is left out of the timing, so the difference is what count / scan /
emit / finish cost on the device).  One box, one run, the variants alternating
call by call; noise_gpu_cs_assign alone is timed in the same loop as the
yardstick.  Shape: 64 Ki connections, one session each, x 16 frames of 1 KiB and
of 64-byte payloads, the frames of a connection back to back (stride 16 x (len +
18)), max_rec = the frames present.  Every timed open starts from the counters
the wire was sealed at (a counter reset, timed alone as well), so that every
frame verifies.  Device-resident, HIP-event timed; GiB/s of payload.
    python tools/bench_framed.py [--out profiles/framed/bench.json]
                                 [--conns N] [--per-conn N] [--lens L ...] [--iters K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "noise-cpp_amd", "python"))
import noise_amd  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "framed", "bench.json"))
    ap.add_argument("--conns", type=int, default=65536)
    ap.add_argument("--per-conn", type=int, default=16)
    ap.add_argument("--lens", type=int, nargs="+", default=[1024, 64])
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    import torch
    noise_amd.load()
    torch.cuda.set_device(0)
    S, P = a.conns, a.per_conn
    R = S * P
    d_keys = torch.empty(S * 32, dtype=torch.uint8, device="cuda")
    noise_amd.fill_synthetic(d_keys, S * 32, 0x4B4559)
    d_sess = torch.arange(S, dtype=torch.int32, device="cuda")
    d_idx = torch.arange(R, dtype=torch.int32, device="cuda") // P  # the records' sessions, for assign alone
    d_zero = torch.zeros(S, dtype=torch.int64, device="cuda")
    tx, txc, rx, rxc = (noise_amd.CipherStateTable(S) for _ in range(4))
    d_scr = torch.empty(R, dtype=torch.int64, device="cuda")
    d_ast = torch.empty(R, dtype=torch.uint8, device="cuda")
    d_nfr = torch.empty(S, dtype=torch.int32, device="cuda")
    d_a, d_b = (torch.empty(S, dtype=torch.int64, device="cuda") for _ in range(2))
    d_cst = torch.empty(S, dtype=torch.uint8, device="cuda")
    rows = []
    for L in a.lens:
        M, W = P * L, P * (L + 18)  # a connection's message and wire bytes
        d_msg = torch.empty(S * M, dtype=torch.uint8, device="cuda")
        noise_amd.fill_synthetic(d_msg, S * M, 7)
        d_wire, d_wirec, d_back = (torch.empty(n, dtype=torch.uint8, device="cuda") for n in (S * W, S * W, S * M))
        d_recs, d_wrecs = (torch.empty(R * 48, dtype=torch.uint8, device="cuda") for _ in range(2))
        d_st, d_stc = (torch.empty(R, dtype=torch.uint8, device="cuda") for _ in range(2))
        for t in (tx, txc, rx, rxc):
            t.set(0, S, d_keys)  # counters back to 0
        msg, frames = noise_amd.span(d_msg, stride=M, length=M), noise_amd.span(d_wire, stride=W, length=W)
        back = noise_amd.span(d_back, stride=M)

        def seal():
            tx.seal_framed(d_sess, msg, frames, L, d_recs, d_st, R, d_nfr, d_a, d_b, d_cst, S, len_sum=R * L)

        # ---- the first seal is the control's batch: same counters, same bytes
        d_wire.zero_()
        d_wirec.zero_()
        seal()
        d_crecs = d_recs.clone()  # descriptors built beforehand: in_off, out_off, len, key_idx

        def seal_ctl():
            txc.encrypt_records(d_crecs, R, d_msg, d_wirec, d_status=d_stc, len_sum=R * L)

        seal_ctl()
        torch.cuda.synchronize()
        assert int(d_st.sum()) == 0 and int(d_stc.sum()) == 0 and int(d_cst.sum()) == 0
        assert bool((d_nfr == P).all()) and bool((d_a == M).all()) and bool((d_b == W).all())
        fr, frc = d_wire.view(R, L + 18), d_wirec.view(R, L + 18)
        assert torch.equal(fr[:, 2:], frc[:, 2:])  # the control leaves the two length bytes to the host
        assert bool((fr[:, 0] == (L + 16) >> 8).all()) and bool((fr[:, 1] == (L + 16) & 255).all())
        d_rwire = d_wire.clone()  # what the receiver got: the counters 0 .. P-1 of every session

        def open_():
            rx.set(0, S, None, d_n=d_zero)
            rx.open_framed(d_sess, noise_amd.span(d_rwire, stride=W, length=W), d_wrecs, d_st, R, d_nfr, d_a, d_cst,
                           S, plain=back, d_plain_len=d_b, len_sum=R * L)

        d_back.zero_()
        open_()
        torch.cuda.synchronize()
        assert int(d_st.sum()) == 0 and int(d_cst.sum()) == 0 and torch.equal(d_back, d_msg)
        assert bool((d_nfr == P).all()) and bool((d_a == W).all()) and bool((d_b == M).all())
        d_cwrecs = d_wrecs.clone()  # what the host walk over the lengths would have uploaded

        def open_ctl():
            rxc.set(0, S, None, d_n=d_zero)
            rxc.decrypt_records(d_cwrecs, R, d_rwire, d_back, d_stc, len_sum=R * L)

        def reset():
            rxc.set(0, S, None, d_n=d_zero)

        def assign():
            txc.assign(d_idx, d_scr, R, d_ast)

        d_back.zero_()
        open_ctl()
        torch.cuda.synchronize()
        assert int(d_stc.sum()) == 0 and torch.equal(d_back, d_msg)
        fns = [seal, seal_ctl, assign, open_, open_ctl, reset]
        for _ in range(3):
            for fn in fns:
                fn()
        se, sc, am, op, oc, rs = timed(torch, fns, a.iters)
        torch.cuda.synchronize()
        assert int(d_st.sum()) == 0 and int(d_stc.sum()) == 0 and int(d_ast.sum()) == 0
        assert torch.equal(d_back, d_msg)
        gib = R * L / 2.0 ** 30
        row = {"len": L, "frames": R, "connections": S, "max_rec": R,
               "seal_us": round(se * 1e3, 1), "cs_encrypt_records_us": round(sc * 1e3, 1),
               "seal_extra_us": round((se - sc) * 1e3, 1), "seal_GiBps": round(gib / (se / 1e3), 1),
               "open_us": round(op * 1e3, 1), "cs_decrypt_records_us": round(oc * 1e3, 1),
               "open_extra_us": round((op - oc) * 1e3, 1), "open_GiBps": round(gib / (op / 1e3), 1),
               "assign_us": round(am * 1e3, 1), "counter_reset_us": round(rs * 1e3, 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    for t in (tx, txc, rx, rxc):
        t.close()
    out = {"tool": "tools/bench_framed.py", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "timing": "HIP events, variants alternating in one run; open and its control include a counter reset",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
