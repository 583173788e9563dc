#!/usr/bin/env python3
"""Time per launch of the grammar-mask kernel beside the sampler, and the host mask path's costs (profiles/json_schema.txt).

For a tool-call schema (an enum, a boolean, a string of up to 64 characters, an array of integers) over a synthetic
vocabulary of V byte strings (every single byte, JSON pieces, random words, a 70-byte token), V = 32000 and 151936:

  * the raw op `_engine.grammar_mask` at B = 1 and B = 8, every row in the brace-level state (just behind "{": few
    tokens survive their first byte) or in an in-string state (almost every token walks all of its bytes), and
    `_engine.sample` of the same build with a mask at the same B and V -- device-event time over `--launches`
    back-to-back launches divided by their number, the median (and range) of `--repeats` windows after a warm-up;
  * the host grammar (SchemaGrammar.mask): the first-visit time per state (median and maximum over the DFA's
    states), the memoised time per state, and the memo's bytes once every state was visited.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCHEMA = {"type": "object",
          "properties": {"tool": {"enum": ["fs.read", "fs.write", "net.get", "proc.list"]},
                         "dry_run": {"type": "boolean"},
                         "path": {"type": "string", "maxLength": 64},
                         "args": {"type": "array", "items": {"type": "integer"}, "maxItems": 8}},
          "required": ["tool", "path"]}


def vocabulary(V, seed=0):
    import numpy as np

    rng = np.random.default_rng(seed)
    toks = [b"", b"", b""] + [bytes([c]) for c in range(256)]
    toks += [b'{"', b'":', b'": ', b'",', b'", "', b'"}', b"},", b"[", b"]", b"true", b"false", b"null", b"x" * 70]
    alphabet = np.frombuffer(b'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 {}[]:,."-_/', np.uint8)
    lens = rng.integers(1, 13, V)
    while len(toks) < V:
        toks.append(bytes(rng.choice(alphabet, int(lens[len(toks)]))))
    return toks[:V], [2]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--vocab", type=int, nargs="*", default=[32000, 151936])
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args(argv)

    import numpy as np

    from aios_amd.runtime import json_schema as JS

    t0 = time.perf_counter()
    dfa = JS.compile_schema(SCHEMA)
    print(f"schema: {dfa.n_states} states x {dfa.n_classes} classes, compiled in {(time.perf_counter() - t0) * 1e3:.1f} ms, "
          f"table {dfa.trans.nbytes + 256 + dfa.n_states} bytes", flush=True)
    brace = dfa.step(1, b"{")
    string = dfa.step(1, b'{"tool":"fs.read","path":"ab')
    assert brace and string

    for V in a.vocab:
        tokens, eos = vocabulary(V)
        vocab = JS.Vocab(tokens, eos)
        g = JS.SchemaGrammar(dfa, vocab)
        first = []
        for s in range(1, dfa.n_states):
            t0 = time.perf_counter()
            g.mask_of(s)
            first.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for s in range(1, dfa.n_states):
            g.mask_of(s)
        memo_us = (time.perf_counter() - t0) * 1e6 / (dfa.n_states - 1)
        print(f"host V={V}: first visit {statistics.median(first):.2f} ms median, {max(first):.2f} ms max per state "
              f"({sum(first):.0f} ms for all {dfa.n_states - 1}); memoised {memo_us:.2f} us per state; memo "
              f"{g.memo_bytes / 1e6:.2f} MB ({(V + 7) // 8} bytes per state)", flush=True)
        if a.host_only:
            continue

        import torch

        from aios_amd.runtime import native

        E = native.require()
        st = torch.cuda.current_stream().cuda_stream
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
        off = np.zeros(V + 1, np.int32)
        off[1:] = np.cumsum([len(t) for t in tokens])
        d_off, d_bytes = dev(off), dev(np.frombuffer(b"".join(tokens), np.uint8).copy())
        bc, tr, ac = dev(dfa.byte_class), dev(dfa.trans.view(np.int16)), dev(dfa.accept)
        tables = dev(np.frombuffer(E.grammar_tables([(bc.data_ptr(), tr.data_ptr(), ac.data_ptr(), dfa.n_states,
                                                       dfa.n_classes)]), np.uint8).copy())
        nb = (V + 7) // 8

        def timed(fn):
            def window():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.launches):
                    fn(i)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e3 / a.launches
            window()
            us = [window() for _ in range(a.repeats)]
            return f"{statistics.median(us):7.2f} us/launch (min {min(us):.2f}, max {max(us):.2f})"

        for B in (1, 8):
            mask = torch.zeros(B, nb, dtype=torch.uint8, device="cuda")
            gid = torch.zeros(B, dtype=torch.int32, device="cuda")
            for name, s in (("brace-level", brace), ("in-string", string)):
                state = torch.full((B,), s, dtype=torch.int32, device="cuda")
                r = timed(lambda i: E.grammar_mask(d_off.data_ptr(), d_bytes.data_ptr(), V, tables.data_ptr(), 1, gid.data_ptr(),
                                                   state.data_ptr(), mask.data_ptr(), B, True, eos, st))
                allowed = int(np.unpackbits(mask[0].cpu().numpy()).sum())
                print(f"gpu  V={V} B={B} grammar_mask {name:12s} {r}  [{allowed} tokens allowed]", flush=True)
            logits = (torch.randn(B, V, generator=torch.Generator().manual_seed(B)) * 2).cuda()
            temp = torch.full((B,), 0.8, device="cuda")
            tk = torch.full((B,), 40, dtype=torch.int32, device="cuda")
            tp = torch.full((B,), 0.95, device="cuda")
            pos = torch.arange(B, dtype=torch.int32, device="cuda")
            tok = torch.zeros(B, dtype=torch.int32, device="cuda")
            r = timed(lambda i: E.sample(logits.data_ptr(), V, B, V, temp.data_ptr(), tk.data_ptr(), 17 + i, tok.data_ptr(),
                                         pos.data_ptr(), mask.data_ptr(), st, tp.data_ptr()))
            print(f"gpu  V={V} B={B} sample (masked, T 0.8, top-k 40, top-p 0.95) {r}", flush=True)


if __name__ == "__main__":
    main()
