"""Host-side checks of the causal decoder variant: the interval rule ego_compact_causal applies on the device
(`masking.causal_decoder_intervals` restates it in numpy) against the reference's dense mask - the one the real reference
recorded in tests/golden/b2_causal.npz, and a numpy restatement of `adapt_decoder_attention_mask` with
`decoder_causal_mask=True` (egom2p/models/egom2p_model.py:446-481) on random geometries - and the registry."""
import numpy as np

from conftest import load_golden
from egom2p_amd.masking import causal_decoder_intervals

CAUSAL_NAME = "egom2p_base_12e_12d_swiglu_nobias_causal"


def _dense(ks, ke, M):
    """intervals -> the reference's boolean mask (True = blocked)"""
    j = np.arange(M)[None, None, :]
    return ~((j >= ks[:, :, None]) & (j < ke[:, :, None]))


def _adapt_causal(mod_mask_pre):
    """adapt_decoder_attention_mask with decoder_causal_mask and decoder_sep_mask: triu(1) | (mod_mask differs), on the modality
    ids BEFORE the padding rows' are set to -1 (forward_mask_decoder calls it first, :437-438)."""
    M = mod_mask_pre.shape[1]
    causal = np.triu(np.ones((M, M), bool), 1)[None]
    sep = mod_mask_pre[:, None, :] != mod_mask_pre[:, :, None]
    return causal | sep


def test_causal_intervals_equal_the_recorded_reference_mask():
    g, meta = load_golden("b2_causal")
    M = meta["n_dec"]
    blocked = np.unpackbits(g["dec_attn_mask_packed"], axis=-1)[:, :, :M].astype(bool)
    ks, ke = causal_decoder_intervals(g["dec_mod_mask"])
    valid = ~g["dec_pad"]
    assert valid[0].all() and 0 < valid[1].sum() < M                    # the fixture has a full sample and one with padding rows
    assert np.array_equal(_dense(ks, ke, M)[valid], blocked[valid])
    # the geometry the fixture is there for: a group across two 128-row query tiles and three 64-key tiles, and a one-row group
    sizes = [int((g["dec_mod_mask"][b] == i).sum()) for b in range(2) for i in np.unique(g["dec_mod_mask"][b]) if i >= 0]
    assert max(sizes) >= 193 and 1 in sizes


def test_causal_intervals_equal_the_reference_rule_on_random_geometries():
    rng = np.random.default_rng(7)
    ids = np.array([11, 22, 33, 44, 55])
    for _ in range(50):
        B, n_mods = 3, int(rng.integers(1, 6))
        M = int(rng.integers(1, 200))
        pre = np.zeros((B, M), np.int64)
        post = np.full((B, M), -1, np.int64)
        for b in range(B):
            order = rng.permutation(ids[:n_mods])
            n_pad = int(rng.integers(0, M + 1)) if rng.random() < 0.7 else 0
            cuts = np.sort(rng.integers(0, M - n_pad + 1, n_mods - 1))
            counts = np.diff(np.concatenate([[0], cuts, [M - n_pad]]))          # target counts per modality, zeros and ones included
            row = np.concatenate([np.full(c, m) for c, m in zip(counts, order)]) if M - n_pad else np.zeros(0, np.int64)
            pre[b, :M - n_pad] = post[b, :M - n_pad] = row
            # padding rows: masked positions in position order - they carry the ids of whichever modalities they fall in
            pre[b, M - n_pad:] = order[np.sort(rng.integers(0, n_mods, n_pad))]
        ks, ke = causal_decoder_intervals(post)
        valid = post >= 0
        assert np.array_equal(_dense(ks, ke, M)[valid], _adapt_causal(pre)[valid])
        assert (ks[~valid] == 0).all() and np.array_equal(ke[~valid], np.broadcast_to(valid.sum(1)[:, None], post.shape)[~valid])


def test_causal_variant_is_registered():
    from egom2p_amd import model
    assert CAUSAL_NAME in model.list_models()
    fn = model.model_entrypoint(CAUSAL_NAME)
    stub = model._unsupported("x", "y")
    assert fn.__code__ is not stub.__code__                              # no longer the refusing stub
    assert fn.__closure__ is not None and any(isinstance(c.cell_contents, dict) and c.cell_contents.get("decoder_causal_mask") is True
                                              for c in fn.__closure__)
