"""Subprocess of tests/test_gpu_edges.py: the engine with kernel-variant knobs given as NAME=VALUE
arguments (GBLS_LANE_R28=0: k_g2_check, the engine-form membership chain; GBLS_LANE_MIN=1025: the
lane clearing chains for the 1100-message launch), read through GBLS_INIT_TUNING.  The remaining
arguments name what to run:

  member      gbls_g2_validate over tests/edges_cases.py g2_membership_cases()
  verdicts    Signature.verify and fast_aggregate_verify (the decode-then-check path) of a valid
              signature, of small-order points alone and of signature + small-order point
  h2c=FILE    gbls_hash_to_g2 of padded_messages() under the POP DST, the raw points to FILE

It prints one JSON line of raw results; the parent holds every expectation."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SK = (0x1ED6E5).to_bytes(32, "big")  # the signers of the verdict cases
SK2 = (0x2ED6E5).to_bytes(32, "big")
MSG = bytes(range(32))


def ref_lib():
    C = ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", "libbls_ref.so"))
    C.ref_sign.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    C.ref_sk_to_pk.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    C.ref_hash_to_g2.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    return C


def ref_sign(C, sk, msg):
    out = ctypes.create_string_buffer(192)
    C.ref_sign(sk, msg, len(msg), out)
    return out.raw


def ref_pk(C, sk):
    out = ctypes.create_string_buffer(96)
    C.ref_sk_to_pk(sk, out)
    return out.raw


def verdict_cases(C):
    """[(label, compressed signature, expected verify, expected fast_aggregate_verify)]: one
    signer for verify, two for fast_aggregate_verify (the aggregate of both signatures)."""
    import edges_cases as E
    from oracle import bls12_381 as O
    s1 = E.g2_of(ref_sign(C, SK, MSG))
    s12 = O.g2_add(s1, E.g2_of(ref_sign(C, SK2, MSG)))
    out = [("valid", O.g2_compress(s1), O.g2_compress(s12), True)]
    for c in E.gold("small_order")["e2"]:
        t = E.g2_of_rec(c["T"])
        out.append(("order %d alone" % c["order"], O.g2_compress(t), O.g2_compress(t), False))
        out.append(("signature + order %d" % c["order"], O.g2_compress(O.g2_add(s1, t)),
                    O.g2_compress(O.g2_add(s12, t)), False))
    return out


def main():
    tasks = []
    for kv in sys.argv[1:]:
        if kv.startswith("GBLS_"):
            k, v = kv.split("=", 1)
            os.environ[k] = v
        else:
            tasks.append(kv)
    from grandine_amd import _lib as G
    G.enable_tuning()  # the engine reads the knobs set above
    from grandine_amd import bls as B
    import edges_cases as E
    L = G.lib()
    res = {"knobs": [a for a in sys.argv[1:] if a.startswith("GBLS_")]}
    for task in tasks:
        if task == "member":
            cases = E.g2_membership_cases()
            st = G.i32_array(len(cases))
            for i in range(len(cases)):
                st[i] = 77
            G.check(L.gbls_g2_validate(G.buf(b"".join(E.g2_b(p) for _, p, _ in cases)), len(cases), st), "validate")
            res["member"] = [st[i] for i in range(len(cases))]
        elif task == "verdicts":
            C = ref_lib()
            pk1, pk2 = B.PublicKey(ref_pk(C, SK)), B.PublicKey(ref_pk(C, SK2))
            got = []
            for label, one, two, _ in verdict_cases(C):
                got.append([label, B.Signature.try_from(one).verify(MSG, pk1),
                            B.Signature.try_from(two).fast_aggregate_verify(MSG, [pk1, pk2])])
            res["verdicts"] = got
        elif task.startswith("h2c="):
            data, off = E.pack(E.padded_messages())
            n = len(off) - 1
            out = ctypes.create_string_buffer(192 * n)
            G.check(L.gbls_hash_to_g2(G.buf(data), G.u32_array(off), n, None, 0, out), "h2c")
            with open(task[4:], "wb") as fh:
                fh.write(out.raw)
            res["h2c"] = n
        else:
            raise SystemExit("unknown task " + task)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
