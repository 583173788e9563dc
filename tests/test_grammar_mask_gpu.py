"""The grammar-mask kernel (csrc/kernels/grammar_mask.hip) against the host rule, byte for byte: every state of
three DFAs at V = 1000 (the last mask byte and the last 64-bit ballot have tails), 4096 and 151,936, over
vocabularies with empty tokens, single bytes, UTF-8 characters split across tokens, a 70-byte token and two
end-of-sequence ids; and the rows without a grammar (gid = -1), with and without a host mask."""
import numpy as np
import pytest

import schema_oracle as SO
from aios_amd.runtime import json_schema as JS

pytestmark = pytest.mark.gpu

DFAS = ("object", "string_bounds", "enum")
EOS = (2, 7)


@pytest.fixture(scope="module")
def native():
    from aios_amd.runtime import native as N

    return N.load(build_if_missing=False)


@pytest.fixture(scope="module")
def dfas():
    return [JS.compile_schema(SO.SCHEMAS[k]) for k in DFAS]


class Device:
    """a vocabulary and the three grammars on the device, through the raw binding"""

    def __init__(self, native, dfas, V):
        import torch

        self.torch, self.native, self.V = torch, native, V
        self.tokens, self.eos = SO.make_vocab(V, seed=V, eos=EOS)
        self.vocab = JS.Vocab(self.tokens, self.eos)
        off = np.zeros(V + 1, np.int32)
        off[1:] = np.cumsum([len(t) for t in self.tokens])
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        self.off = dev(off)
        self.bytes = dev(np.frombuffer(b"".join(self.tokens), np.uint8).copy())
        self.keep, grammars = [], []
        for d in dfas:
            assert d.trans.max() < d.n_states and d.byte_class.max() < d.n_classes  # (the kernel does not check)
            bc, tr, ac = dev(d.byte_class), dev(d.trans.view(np.int16)), dev(d.accept)
            self.keep += [bc, tr, ac]
            grammars.append((bc.data_ptr(), tr.data_ptr(), ac.data_ptr(), d.n_states, d.n_classes))
        self.tables = dev(np.frombuffer(native.grammar_tables(grammars), np.uint8).copy())  # the launch's table array
        self.n_grammars = len(grammars)
        self.nb = (V + 7) // 8

    def run(self, gids, states, fill_free, poison=0xAA):
        torch = self.torch
        B = len(gids)
        mask = torch.full((B + 1, self.nb), poison, dtype=torch.uint8, device="cuda")  # (a guard row behind the last)
        g = torch.tensor(gids, dtype=torch.int32, device="cuda")
        s = torch.tensor(states, dtype=torch.int32, device="cuda")
        self.native.grammar_mask(self.off.data_ptr(), self.bytes.data_ptr(), self.V, self.tables.data_ptr(), self.n_grammars,
                                 g.data_ptr(),
                                 s.data_ptr(), mask.data_ptr(), B, fill_free, list(self.eos),
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out = mask.cpu().numpy()
        assert (out[B] == poison).all()  # nothing is written behind the last row
        return out[:B]


@pytest.fixture(scope="module", params=[1000, 4096, 151936])
def device(request, native, dfas):
    return Device(native, dfas, request.param)


def test_vocabulary_has_the_hard_tokens(device):
    lens = [len(t) for t in device.tokens]
    assert max(lens) == 70 and lens.count(0) >= 3 and all(device.tokens[e] == b"" for e in EOS)
    assert "中".encode()[:1] in device.tokens and "中".encode()[1:] in device.tokens and b"\xc0\x80" in device.tokens


@pytest.mark.parametrize("which", range(len(DFAS)), ids=DFAS)
def test_every_state_equals_the_host_rule(device, dfas, which):
    d = dfas[which]
    g = JS.SchemaGrammar(d, device.vocab)
    states = list(range(d.n_states))  # (the dead state 0 included: it allows nothing)
    got = device.run([which] * len(states), states, True)
    want = np.stack([np.frombuffer(g.mask_of(s), np.uint8) for s in states])
    bad = np.nonzero((got != want).any(axis=1))[0]
    print(f"V={device.V} {DFAS[which]}: {len(states)} states, {int(want.sum(dtype=np.int64))} mask-byte sum, "
          f"{len(bad)} rows differ")
    assert (got == want).all(), bad[:10]
    assert not got[0].any()
    if device.V % 8:
        assert not (got[:, -1] >> (device.V % 8)).any()  # bits past V
    # the end-of-sequence ids follow accept, whatever else the state allows
    for e in EOS:
        assert ((got[:, e >> 3] >> (e & 7)) & 1).tolist() == d.accept.tolist()


def test_one_row_matches_the_brute_force_rule(native, dfas):
    """B = 1, and the oracle's oracle: token-by-token stepping, on the small vocabulary"""
    device = Device(native, dfas, 1000)
    d = dfas[0]
    for s in (1, d.n_states // 2, d.n_states - 1):
        got = device.run([0], [s], True)
        assert got[0].tobytes() == SO.brute_mask(d, device.tokens, device.eos, s)


@pytest.mark.parametrize("host_mask", [True, False])
def test_rows_without_a_grammar(device, dfas, host_mask):
    """B = 8, grammars and free rows mixed: with a host mask the free rows keep its bytes (0xAA here), without
    one they become all ones with the bits past V zero"""
    gids = [-1, 0, 1, -1, -1, 2, 0, -1]
    states = [0, 1, 5, 3, 0, 2, 7, 1]
    got = device.run(gids, states, fill_free=not host_mask)
    ones = np.packbits(np.ones(device.V, np.uint8), bitorder="little")
    for b, (gid, s) in enumerate(zip(gids, states)):
        if gid >= 0:
            assert got[b].tobytes() == JS.SchemaGrammar(dfas[gid], device.vocab).mask_of(s), b
        elif host_mask:
            assert (got[b] == 0xAA).all(), b
        else:
            assert (got[b] == ones).all(), b
    # a grammar id the launch does not have, and a state outside the table: nothing allowed
    got = device.run([3, 0], [1, dfas[0].n_states], True)
    assert not got.any()
