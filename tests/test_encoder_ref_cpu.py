"""CPU: tests/encoder_ref.py, the reference of tests/test_encoder_fp64_gpu.py, held to account on its own.

1. The float64 reference equals oracle.rmcl_oracle.infer in float64 to 1e-12 relative on text_feats, image_feats and the masks, at one dense case
   (the shape of case J, every patch valid) and one ragged case (case D, its explicit selection handed to the oracle): a wrong reference cannot
   then bless a wrong kernel.
2. Arena packing round-trips through runtime.param_specs on rmcl_param_layout's offsets.
3. The rounding model of the bf16 arms is capped.  The GPU tests allow a kernel 3 x the model's worst-row deviation from float64 on the same
   case; MODEL_CAPS (tests/encoder_cases.py) holds the model alone to twice the figure measured on the CPU when this test was written
   (MODEL_MEASURED: per variant and per block, every layer's tensors on their own), so that "3 x model" cannot drift loose.
   Largest measured figure per variant:
     J:data 3.8e-3 (dpatches)   J:full 1.8e-2 (qkv weight gradient)   K:infer 3.9e-3 (xn image rows)   K:data 4.7e-3 (dpatches)
     K and K2 with the fold taken: 4.0e-3 .. 5.6e-3
     K:full 1.3e-2   L4:full 1.9e-2   L3:full 2.0e-2 (qkv weight gradient each); xn itself: 2.3e-4 .. 1.1e-3 (text rows), up to 4.0e-3 (image rows).
   profiles/encoder_parity.json carries the same figures next to the kernel's.
4. The cases hold what they claim: every sample has a valid key, every ragged sample a valid patch, case A has the pad id, ids repeated within
   and across samples and a sample with one valid token, the replaced sets are none / some / all, an output side of 1 and a missing image exist."""
import ctypes as C

import pytest
import torch

from oracle import rmcl_oracle as O
from tests import encoder_cases as T
from tests import encoder_ref as R
from tests.encoder_cases import BF16_VARIANTS, MODEL_CAPS, get_case, model_figures


def _image_of(c):
    """[B, 3, S, S] whose 8 x 8 patches are the rows of a dense case."""
    d = c.dims
    g = int(round(d.P ** 0.5))
    assert g * g == d.P
    return c.patches.double().view(d.B, g, g, 3, 8, 8).permute(0, 3, 1, 4, 2, 5).reshape(d.B, 3, 8 * g, 8 * g)


@pytest.mark.parametrize("name", ["J", "D"])
def test_reference_agrees_with_the_oracle(name):
    c = get_case(name)
    d = c.dims
    arena = c.arena.double()
    p = R.views(arena, c.specs)
    g0 = 4 if c.ragged else int(round(d.P ** 0.5))
    cfg = dict(patch_size=8, image_size=8 * g0, num_layers=d.layers, num_heads=d.H, max_image_len=-1)
    img = c.img.double() if c.ragged else _image_of(c)
    sel = c.ragged["sel"].long() if c.ragged else None
    with torch.no_grad():
        want = O.infer(p, cfg, c.text_ids, c.text_mask, img, select=sel)
        xn, co = R.encoder_ref(arena, c.specs, d, c.text_ids, c.text_mask, c.patches.double(), ragged=c.ragged)
    assert torch.equal(co[:, :d.L].long(), want["text_masks"]) and torch.equal(co[:, d.L:].long(), want["image_masks"])
    for key, got in (("text_feats", xn[:, :d.L]), ("image_feats", xn[:, d.L:])):
        rel = float((got - want[key]).abs().max() / want[key].abs().max())
        print(f"{name} {key}: {rel:.2e}")
        assert rel <= 1e-12, (key, rel)


@pytest.mark.parametrize("name", ["A", "C", "Ep", "K"])
def test_arena_packing_round_trips(name):
    c = get_case(name)
    p = R.views(c.arena, c.specs)
    assert torch.equal(R.pack(p, c.specs, c.total), c.arena)
    # the slots are disjoint, inside the arena, and the ones the encoder reads sit where rmcl_param_layout says
    covered = torch.zeros(c.total, dtype=torch.int32)
    for _, off, shape in c.specs:
        covered[off:off + R.numel(shape)] += 1
    assert int(covered.max()) == 1
    lay, d = c.lay, c.dims
    assert c.offs["text_embeddings.word_embeddings.weight"] == (lay.word, (d.vocab, d.D))
    assert c.offs["token_type_embeddings.weight"] == (lay.vtype, (3 if d.n_types == 3 else 2, d.D))
    assert c.offs["transformer.pos_embed"] == (lay.pos_img, (1, (d.Pp or d.P) + 1, d.D))
    last = f"transformer.blocks.{d.layers - 1}."
    assert c.offs[last + "mlp.fc2.weight"] == (lay.layer0 + (d.layers - 1) * lay.layer_stride + lay.fc2_w, (d.D, d.mlp))
    assert c.offs[last + "attn.qkv.bias"] == (lay.layer0 + (d.layers - 1) * lay.layer_stride + lay.qkv_b, (3 * d.D,))
    assert c.offs["transformer.norm.bias"] == (lay.norm_b, (d.D,))


@pytest.mark.parametrize("label", sorted(BF16_VARIANTS))
def test_rounding_model_stays_within_its_caps(label):
    fig = model_figures(label)
    print(label, {b: float(f"{v:.3e}") for b, v in sorted(fig.items())})
    assert set(fig) == set(MODEL_CAPS[label])
    over = {b: (v, MODEL_CAPS[label][b]) for b, v in fig.items() if not v <= MODEL_CAPS[label][b]}
    assert not over, over


def test_the_cases_hold_what_they_claim():
    for name in T.SHAPES:
        c = get_case(name)
        ref_mask = T.reference(name, "f64", None)["co"]
        assert bool((ref_mask.sum(1) >= 1).all()), name
        assert bool((c.text_mask.sum(1) >= 1).all()), name
        if c.ragged:
            assert bool((c.ragged["counts"] >= 1).all()) and int(c.ragged["counts"].max()) == c.dims.P
            assert int(c.ragged["counts"].min()) < c.dims.P
            assert any(int(h) == 1 for h in c.ragged["hw"][:, 0]) and any(int(w) == 1 for w in c.ragged["hw"][:, 1])
        else:
            assert int(ref_mask[:, c.dims.L:].sum()) >= c.dims.B * c.dims.P      # at most the one pad patch of case A is masked
    a = get_case("A")
    ids, tm = a.text_ids, a.text_mask
    assert bool(((ids == 0) & (tm == 1)).any()) and bool(((ids == 0) & (tm == 0)).any())          # the pad id, attended to and not
    assert any(len(set(r.tolist())) < len(r) for r in ids)                                          # a repeat inside a sample
    assert set(ids[0].tolist()) & set(ids[2].tolist()) - {0}                                        # and across samples
    assert 1 in tm.sum(1).tolist()
    assert int(T.reference("A", "f64", None)["co"][2, -1]) == 0
    assert [sum(r) for r in T.REPLACED_A] == [0, 4, 9]
    i = get_case("I")
    assert any(not 0 <= k < i.dims.B for k in i.rank) and len(set(i.rank)) == len(i.rank)
    for name in ("E2", "Ep"):
        assert get_case(name).dims.n_types == 3
    assert get_case("Ep").dims.B % 2 == 0 and get_case("Ep").dims.img_type == -1
    lay = C.sizeof(get_case("L4").lay)
    assert lay > 0 and get_case("L4").dims.B * get_case("L4").N == 256 and get_case("L3").dims.B * get_case("L3").N == 192
