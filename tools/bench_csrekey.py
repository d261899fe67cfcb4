#!/usr/bin/env python3
"""What the in-band rekey schedule of a CipherState table costs
(noise_gpu_csrekey_set): noise_gpu_cs_{en,de}crypt_sessions on tables with
every = 0 (off), 1000 and 16, on one box in one run, the variants alternating
call by call.  Shape: tools/bench_cstate.py's (BASELINE config 3: 64 Ki
sessions x 16 records, interleaved across sessions) at 1 KiB and at 64-byte
records.  Session s starts at counter s, so that at every = 1000 about 1.6 %
of the sessions cross a boundary in each call; at every = 16 every session
crosses one.  Each timed decrypt opens what the encrypt before it wrote, so
sender and receiver stay in step and every tag verifies.  Device-resident,
HIP-event timed.
    python tools/bench_csrekey.py [--out profiles/csrekey/bench.json]
                                  [--sessions N] [--per-session N] [--lens L ...] [--iters K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "noise-cpp_amd", "python"))
import noise_amd  # noqa: E402
from bench_cstate import timed  # noqa: E402

EVERY = (0, 1000, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csrekey", "bench.json"))
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--per-session", type=int, default=16)
    ap.add_argument("--lens", type=int, nargs="+", default=[1024, 64])
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    import torch
    noise_amd.load()
    torch.cuda.set_device(0)
    S, R = a.sessions, a.sessions * a.per_session
    d_keys = torch.empty(S * 32, dtype=torch.uint8, device="cuda")
    noise_amd.fill_synthetic(d_keys, S * 32, 0x4B4559)
    d_idx = (torch.arange(R, dtype=torch.int64, device="cuda") % S).to(torch.int32)
    d_n0 = torch.arange(S, dtype=torch.int64, device="cuda")
    pairs = []
    for every in EVERY:
        tx, rx = noise_amd.CipherStateTable(S), noise_amd.CipherStateTable(S)
        tx.set_rekey_every(every)
        rx.set_rekey_every(every)
        pairs.append((tx, rx))
    rows = []
    for L in a.lens:
        d_pt = torch.empty(R * L, dtype=torch.uint8, device="cuda")
        noise_amd.fill_synthetic(d_pt, R * L, 7)
        d_ct = torch.empty(R * (L + 16), dtype=torch.uint8, device="cuda")
        d_back = torch.empty(R * L, dtype=torch.uint8, device="cuda")
        d_st = torch.empty(R, dtype=torch.uint8, device="cuda")
        fns = []
        for tx, rx in pairs:
            tx.set(0, S, d_keys, d_n=d_n0)
            rx.set(0, S, d_keys, d_n=d_n0)
            fns.append(lambda tx=tx: tx.encrypt_sessions(d_idx, d_pt, L, d_ct, L + 16, L, R))
            fns.append(lambda rx=rx: rx.decrypt_sessions(d_idx, d_ct, L + 16, d_back, L, L, d_st, R))
        for k in range(0, len(fns), 2):  # every pair round-trips
            d_back.zero_()
            fns[k](), fns[k + 1]()
            torch.cuda.synchronize()
            assert torch.equal(d_pt, d_back) and int(d_st.sum()) == 0, EVERY[k // 2]
        for _ in range(3):
            for fn in fns:
                fn()
        ms = timed(torch, fns, a.iters)
        torch.cuda.synchronize()
        assert torch.equal(d_pt, d_back) and int(d_st.sum()) == 0
        gib = R * L / 2.0 ** 30
        row = {"len": L, "records": R, "sessions": S}
        for k, every in enumerate(EVERY):
            enc, dec = ms[2 * k], ms[2 * k + 1]
            row["every_%d" % every] = {
                "cs_encrypt_us": round(enc * 1e3, 1), "cs_decrypt_us": round(dec * 1e3, 1),
                "cs_encrypt_GiBps": round(gib / (enc / 1e3), 1), "cs_decrypt_GiBps": round(gib / (dec / 1e3), 1),
                "cs_encrypt_extra_us": round((enc - ms[0]) * 1e3, 1),
                "cs_decrypt_extra_us": round((dec - ms[1]) * 1e3, 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    for tx, rx in pairs:
        tx.close()
        rx.close()
    out = {"tool": "tools/bench_csrekey.py", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "timing": "HIP events, variants alternating in one run; extra = against every_0 in the same run",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
