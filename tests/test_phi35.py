"""Phi-3.5-mini-instruct on the host side (no GPU): its config against the reference's record, the head-size gate, and the
HF Phi-3 converter against the reference's own copy_weights_phi (tests/golden/make_golden_hs96.py)."""
import itertools
import json

import pytest
import torch

from conftest import GOLDEN, load_golden
from dualhyp_amd.checkpoint import HFLlamaConverter, HFPhi3Converter, hf_converter
from dualhyp_amd.config import Config


def test_phi35_config_equals_the_reference():
    want = json.loads((GOLDEN / "phi35_config.json").read_text())
    c = Config.from_name("Phi-3.5-mini-instruct")
    got = c.to_dict()
    got["rope_n_elem"] = c.rope_n_elem
    for k, v in want.items():
        assert got[k] == v, f"{k}: {got[k]!r} != reference {v!r}"
    assert Config.from_name("Phi-3.5-mini-instruct").head_size == 96
    assert Config.from_name("Phi-3.5-mini-instruct").n_query_groups == 32


def test_head_size_96_is_supported_and_80_is_not():
    for name in ("Phi-3.5-mini-instruct", "parity-hs96", "parity-hs96-gqa"):
        c = Config.from_name(name)
        c.check_supported()
        assert c.head_size == 96
    with pytest.raises(NotImplementedError, match="head_size"):
        Config.from_name("parity-hs96", n_embd=320).check_supported()        # 4 heads of 80


def _phi3_fixture():
    t, meta = load_golden("convert_hf_phi3")
    hf = {k[3:]: v for k, v in t.items() if k.startswith("hf.")}
    lit = {k[4:]: v for k, v in t.items() if k.startswith("lit.")}
    return hf, lit, meta


def test_phi3_conversion_equals_the_reference_in_any_shard_order():
    hf, lit, meta = _phi3_fixture()
    cfg = Config(**meta["config"])
    names = sorted(hf)
    # three shards (the fixture's split and two others), every order
    late = set(meta["shard2_keys"])
    splits = [[[k for k in names if k not in late], [k for k in names if k in late]],
              [names[0::3], names[1::3], names[2::3]],
              [[k for k in names if ".0." not in k], [k for k in names if ".0." in k]]]
    for split in splits:
        for order in itertools.permutations(split):
            conv = hf_converter(cfg)
            assert isinstance(conv, HFPhi3Converter)
            for shard in order:
                conv.add({k: hf[k] for k in shard})
            got = conv.finish()
            assert sorted(got) == sorted(lit)
            for k, v in lit.items():
                assert torch.equal(got[k], v), k
    # the reference's quirk, pinned: qkv_proj lands in attn.attn as it stands ([Q; K; V], not interleaved per group)
    assert torch.equal(lit["transformer.h.0.attn.attn.weight"], hf["model.layers.0.self_attn.qkv_proj.weight"])


def test_phi3_conversion_refuses_outdated_checkpoints():
    _, _, meta = _phi3_fixture()
    cfg = Config(**meta["config"])
    assert meta["outdated_error"].startswith("You are using an outdated Phi checkpoint")
    for key in ("transformer.h.0.attn.attn.weight", "layers.0.mlp.fc1.weight"):
        with pytest.raises(ValueError, match="outdated Phi checkpoint"):
            HFPhi3Converter(cfg).add({key: torch.zeros(2, 2)})


def test_phi3_conversion_keeps_the_dtype_cast_and_llama_dispatch():
    hf, lit, meta = _phi3_fixture()
    conv = HFPhi3Converter(Config(**meta["config"]), dtype=torch.bfloat16)
    conv.add(hf)
    got = conv.finish()
    assert all(v.dtype == torch.bfloat16 for v in got.values())
    assert torch.equal(got["transformer.h.1.mlp.fc_2.weight"], lit["transformer.h.1.mlp.fc_2.weight"].to(torch.bfloat16))
    assert isinstance(hf_converter(Config.from_name("tiny-llama-1.1b")), HFLlamaConverter)
    with pytest.raises(KeyError, match="unexpected HF Phi-3 tensor"):
        HFPhi3Converter(Config(**meta["config"])).add({"model.layers.0.self_attn.rotary_emb.inv_freq": torch.zeros(2)})
