"""Subprocess of tests/test_gpu_curve28_lane.py: the engine with kernel-variant knobs given as
NAME=VALUE arguments (GBLS_LANE_MIN=1025: the lane kernels for an 1100-set launch;
GBLS_CLEAR_STAGED, GBLS_LANE_R28, GBLS_MSM_MIN, GBLS_MSM_R28), read through GBLS_INIT_TUNING.
Every child is a fresh process.  The remaining arguments name what to run:

  h2c=FILE      gbls_hash_to_g2 of tests/edges_cases.py padded_messages() (1100 messages: 17 full
                waves and 12 lanes), the raw points to FILE
  partial=FILE  gbls_multi_verify_partials_device of factory.c2_batch(1100) as ONE segment: the 576
                partial bytes to FILE, the error word in the JSON line
  special=FILE  the "special" case of tests/gpu_msm_windows.py (equal points and a cancelling pair
                in one bucket; 3 segments) through gbls_multi_verify_partials_device: 3 x 576 bytes

After each task the stage timers' call counts since the last reset go into the JSON line, so the
parent can assert the path and not only the bytes.  It prints one JSON line."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_SETS = 1100
SEED = 2828


def stage_calls(L):
    calls = (ctypes.c_uint32 * 64)()
    ns = L.gbls_profile_read(None, calls, 64)
    out = {L.gbls_stage_name(i).decode(): int(calls[i]) for i in range(ns)}
    L.gbls_profile_reset()
    return out


def partials(G, L, msgs, sigs, pks, rands, off):
    import torch

    dev = torch.device("cuda", 0)
    n, nseg = off[-1], len(off) - 1
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    m, s, p = up(msgs[:32 * n]), up(sigs[:192 * n]), up(pks[:96 * n])
    r = torch.tensor([x - (1 << 64) if x >= 1 << 63 else x for x in rands[:n]], dtype=torch.int64, device=dev)
    parts = torch.zeros(nseg * 576, dtype=torch.uint8, device=dev)
    errs = torch.full((nseg,), -1, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    G.check(L.gbls_multi_verify_partials_device(m.data_ptr(), s.data_ptr(), p.data_ptr(), r.data_ptr(), n,
                                                G.u32_array(off), nseg, parts.data_ptr(), errs.data_ptr(), st),
            "partials")
    torch.cuda.synchronize()
    return bytes(parts.cpu().numpy()), [int(x) for x in errs.cpu()]


def main():
    tasks = []
    for kv in sys.argv[1:]:
        if kv.startswith("GBLS_"):
            k, v = kv.split("=", 1)
            os.environ[k] = v
        else:
            tasks.append(kv)
    if any(t.startswith("special=") for t in tasks):
        assert os.environ.get("GBLS_MSM_MIN") == "1"
        import gpu_msm_windows as W  # its plan; it sets GBLS_MSM_MIN=1 itself as well
    from grandine_amd import _lib as G
    G.enable_tuning()  # the engine reads the knobs set above
    L = G.lib()
    L.gbls_profile(1)
    L.gbls_profile_reset()
    res = {"knobs": [a for a in sys.argv[1:] if a.startswith("GBLS_")], "stages": {}}
    for task in tasks:
        name, path = task.split("=", 1)
        if name == "h2c":
            import edges_cases as E
            data, off = E.pack(E.padded_messages())
            n = len(off) - 1
            out = ctypes.create_string_buffer(192 * n)
            G.check(L.gbls_hash_to_g2(G.buf(data), G.u32_array(off), n, None, 0, out), "h2c")
            raw, res["h2c"] = out.raw, n
        elif name == "partial":
            from grandine_amd import factory as F
            msgs, sigs, pks, rands = F.c2_batch(N_SETS, seed=SEED)
            raw, res["partial_err"] = partials(G, L, msgs, sigs, pks, rands, [0, N_SETS])
        elif name == "special":
            case = next(c for c in W.plan(W.Oracle()) if c[0] == "special")
            _, sets, off, _ = case
            raw, res["special_err"] = partials(G, L, b"".join(x[0] for x in sets), b"".join(x[1] for x in sets),
                                               b"".join(x[2] for x in sets), [x[3] for x in sets], off)
        else:
            raise SystemExit("unknown task " + task)
        with open(path, "wb") as fh:
            fh.write(raw)
        res["stages"][name] = stage_calls(L)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
