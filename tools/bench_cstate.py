#!/usr/bin/env python3
"""What nonce assignment on the GPU costs: noise_gpu_cs_{en,de}crypt_sessions
(a device-resident CipherState table assigns the nonces, then the sessions
kernels run) against noise_gpu_{en,de}crypt_sessions with nonces precomputed
on the host and already resident, on one box in one run, the two variants
alternating call by call.  Shape: BASELINE config 3 (64 Ki sessions x 16
records, interleaved across sessions) at 1 KiB and at 64-byte records, where
assignment weighs most; plus noise_gpu_cs_assign alone.  Device-resident,
HIP-event timed; GiB/s of plaintext per direction.
    python tools/bench_cstate.py [--out profiles/cstate/bench.json]
                                 [--sessions N] [--per-session N] [--lens L ...] [--iters K]

--window measures the out-of-order receive instead (replay windows,
noise_gpu_cswin_decrypt_sessions): the same shape with the wire order shuffled
inside every session, alternating with the stateless decrypt of the same
records and with noise_gpu_cs_decrypt_sessions; plus a skewed batch, 2^16
verified copies of one record of one session, which is the longest ordered
walk a batch of that size can ask for.  Every timed windowed call starts from
fresh windows (a reset, timed alone as well), so that every record is
decrypted and accepted.
    python tools/bench_cstate.py --window [--out profiles/cswin/bench.json]"""
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


def window_leg(torch, a):
    S, P = a.sessions, a.per_session
    R = S * P
    d_keys = torch.empty(S * 32, dtype=torch.uint8, device="cuda")
    noise_amd.fill_synthetic(d_keys, S * 32, 0x4B4559)
    i = torch.arange(R, dtype=torch.int64, device="cuda")
    d_idx = (i % S).to(torch.int32)
    d_non = i // S
    # the wire: record k of a session carries a nonce drawn from a permutation of its P nonces
    gen = torch.Generator(device="cuda").manual_seed(1)
    perm = torch.rand(S, P, device="cuda", generator=gen).argsort(dim=1)
    d_wire = perm.t().contiguous().reshape(-1).to(torch.int64)
    tx, rx, wx = (noise_amd.CipherStateTable(S) for _ in range(3))
    rows = []
    for L in a.lens:
        d_pt = torch.empty(R * L, dtype=torch.uint8, device="cuda")
        noise_amd.fill_synthetic(d_pt, R * L, 7)
        d_ct = torch.empty(R * (L + 16), dtype=torch.uint8, device="cuda")
        d_ct2 = torch.empty(R * (L + 16), dtype=torch.uint8, device="cuda")
        d_back = torch.empty(R * L, dtype=torch.uint8, device="cuda")
        d_st = torch.empty(R, dtype=torch.uint8, device="cuda")
        for t in (tx, rx, wx):
            t.set(0, S, d_keys)
        noise_amd.encrypt_sessions(d_keys, S, d_idx, d_wire, d_pt, L, d_ct, L + 16, L, R)

        def base_dec():
            noise_amd.decrypt_sessions(d_keys, S, d_idx, d_wire, d_ct, L + 16, d_back, L, L, d_st, R)

        def cs_enc():
            tx.encrypt_sessions(d_idx, d_pt, L, d_ct2, L + 16, L, R)

        def cs_dec():
            rx.decrypt_sessions(d_idx, d_ct2, L + 16, d_back, L, L, d_st, R)

        def reset():
            wx.window_reset(0, S)

        def win_dec():
            wx.window_reset(0, S)
            wx.decrypt_sessions_window(d_idx, d_wire, d_ct, L + 16, d_back, L, L, d_st, R)

        for fn in (base_dec, cs_dec, win_dec):
            if fn is cs_dec:
                cs_enc()
            d_back.zero_()
            fn()
            torch.cuda.synchronize()
            assert torch.equal(d_pt, d_back) and int(d_st.sum()) == 0, fn.__name__
        for _ in range(3):
            base_dec(), cs_enc(), cs_dec(), win_dec()
        bd, _, cd, wd, rs = timed(torch, [base_dec, cs_enc, cs_dec, win_dec, reset], a.iters)
        torch.cuda.synchronize()
        assert torch.equal(d_pt, d_back) and int(d_st.sum()) == 0
        gib = R * L / 2.0 ** 30
        row = {"len": L, "records": R, "sessions": S, "order": "shuffled inside each session",
               "sessions_decrypt_GiBps": round(gib / (bd / 1e3), 1),
               "cs_decrypt_GiBps": round(gib / (cd / 1e3), 1),
               "window_decrypt_GiBps": round(gib / (wd / 1e3), 1),
               "cs_decrypt_extra_us": round((cd - bd) * 1e3, 1),
               "window_decrypt_extra_us": round((wd - bd) * 1e3, 1),
               "window_reset_us": round(rs * 1e3, 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        # skewed: K verified copies of one record of one session
        K = 1 << 16
        d_idx1 = torch.full((K,), 5, dtype=torch.int32, device="cuda")
        d_non1 = torch.full((K,), 3, dtype=torch.int64, device="cuda")
        noise_amd.encrypt_sessions(d_keys, S, d_idx1[:1], d_non1[:1], d_pt, L, d_ct2, L + 16, L, 1)
        d_ct2[:K * (L + 16)].view(K, L + 16)[1:] = d_ct2[:L + 16]

        def skew_base():
            noise_amd.decrypt_sessions(d_keys, S, d_idx1, d_non1, d_ct2, L + 16, d_back, L, L, d_st, K)

        def skew_win():
            wx.window_reset(5, 1)
            wx.decrypt_sessions_window(d_idx1, d_non1, d_ct2, L + 16, d_back, L, L, d_st, K)

        skew_base(), skew_win()
        torch.cuda.synchronize()
        st = d_st[:K]
        assert int(st[0]) == 0 and bool((st[1:] == noise_amd.REC_REPLAY).all())
        assert torch.equal(d_back[:L], d_pt[:L]) and int(d_back[L:K * L].max()) == 0
        sb, sw = timed(torch, [skew_base, skew_win], a.iters)
        row = {"len": L, "records": K, "sessions": 1, "order": "copies of one verified record",
               "sessions_decrypt_us": round(sb * 1e3, 1), "window_decrypt_us": round(sw * 1e3, 1),
               "window_decrypt_extra_us": round((sw - sb) * 1e3, 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    for t in (tx, rx, wx):
        t.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", action="store_true", help="the replay-window leg (profiles/cswin/bench.json)")
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--per-session", type=int, default=16)
    ap.add_argument("--lens", type=int, nargs="+", default=[1024, 64])
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "cswin" if a.window else "cstate", "bench.json")
    import torch
    noise_amd.load()
    torch.cuda.set_device(0)
    if a.window:
        write(a, torch, window_leg(torch, a))
        return
    S, R = a.sessions, a.sessions * a.per_session
    d_keys = torch.empty(S * 32, dtype=torch.uint8, device="cuda")
    noise_amd.fill_synthetic(d_keys, S * 32, 0x4B4559)
    i = torch.arange(R, dtype=torch.int64, device="cuda")
    d_idx = (i % S).to(torch.int32)  # interleaved: consecutive records belong to different sessions
    d_non = i // S                   # what a host walk over the batch would have uploaded
    tx, rx = noise_amd.CipherStateTable(S), noise_amd.CipherStateTable(S)
    d_scr = torch.empty(R, dtype=torch.int64, device="cuda")
    d_ast = torch.empty(R, dtype=torch.uint8, device="cuda")
    rows = []
    for L in a.lens:
        d_pt = torch.empty(R * L, dtype=torch.uint8, device="cuda")
        noise_amd.fill_synthetic(d_pt, R * L, 7)
        d_ct = torch.empty(R * (L + 16), dtype=torch.uint8, device="cuda")
        d_ct2 = torch.empty(R * (L + 16), dtype=torch.uint8, device="cuda")
        d_back = torch.empty(R * L, dtype=torch.uint8, device="cuda")
        d_st = torch.empty(R, dtype=torch.uint8, device="cuda")
        for t in (tx, rx):
            t.set(0, S, d_keys)  # counters back to 0: both sides in step

        def base_enc():
            noise_amd.encrypt_sessions(d_keys, S, d_idx, d_non, d_pt, L, d_ct, L + 16, L, R)

        def base_dec():
            noise_amd.decrypt_sessions(d_keys, S, d_idx, d_non, d_ct, L + 16, d_back, L, L, d_st, R)

        def cs_enc():
            tx.encrypt_sessions(d_idx, d_pt, L, d_ct2, L + 16, L, R)

        def cs_dec():
            rx.decrypt_sessions(d_idx, d_ct2, L + 16, d_back, L, L, d_st, R)

        def assign():
            tx.assign(d_idx, d_scr, R, d_ast)

        # the table's first batch (n = 0) is the precomputed batch: same bytes
        cs_enc()
        base_enc()
        cs_dec()
        torch.cuda.synchronize()
        assert torch.equal(d_ct, d_ct2) and torch.equal(d_pt, d_back) and int(d_st.sum()) == 0
        for _ in range(5):
            base_enc(), base_dec(), cs_enc(), cs_dec()
        torch.cuda.synchronize()
        assert torch.equal(d_pt, d_back) and int(d_st.sum()) == 0
        be, bd, ce, cd = timed(torch, [base_enc, base_dec, cs_enc, cs_dec], a.iters)
        tx.set(0, S, d_keys)
        assign()
        (am,) = timed(torch, [assign], a.iters)
        torch.cuda.synchronize()
        assert int(d_ast.sum()) == 0
        gib = R * L / 2.0 ** 30
        row = {"len": L, "records": R, "sessions": S,
               "sessions_encrypt_GiBps": round(gib / (be / 1e3), 1),
               "sessions_decrypt_GiBps": round(gib / (bd / 1e3), 1),
               "cs_encrypt_GiBps": round(gib / (ce / 1e3), 1),
               "cs_decrypt_GiBps": round(gib / (cd / 1e3), 1),
               "cs_encrypt_extra_us": round((ce - be) * 1e3, 1),
               "cs_decrypt_extra_us": round((cd - bd) * 1e3, 1),
               "assign_us": round(am * 1e3, 1),
               "assign_Mrec_per_s": round(R / (am / 1e3) / 1e6, 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    tx.close()
    rx.close()
    write(a, torch, rows)


def write(a, torch, rows):
    out = {"tool": "tools/bench_cstate.py" + (" --window" if a.window else ""),
           "device": torch.cuda.get_device_name(0),
           "iters": a.iters, "timing": "HIP events, variants alternating in one run", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
