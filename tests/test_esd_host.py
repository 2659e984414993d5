"""ESD's host side (pdm/utils/esd.py, no GPU): pairs, the checkpoint's name and nesting, the three draws, the timestep of the
predictions, which modules a --train_method trains and where they lie in the arena."""
import numpy as np
import pytest
import torch


def _tiny_entries():
    from pdm.models.unet import params, spec
    cfg = spec.UNetConfig.tiny()
    av = spec.arch_vector_for_budget(cfg, 0.6, hw=16)[0]
    return params.build_entries(cfg, spec.apply_arch_vector(cfg, av))


def test_pairs():
    from pdm.utils import esd as E
    assert E.build_pairs("Van Gogh") == [["Van Gogh", "Van Gogh"]]
    assert E.build_pairs("Van Gogh", "art") == [["Van Gogh", "art"]]
    assert E.build_pairs("nudity, violence") == [["nudity", "nudity"], ["violence", "violence"]]
    assert E.build_pairs("nudity, violence , gore", " person") == [["nudity", "person"], ["violence", "person"], ["gore", "person"]]
    assert E.build_pairs("a,b", "c,d") == [["a", "c"], ["b", "d"]]
    with pytest.raises(Exception, match="length"):
        E.build_pairs("a,b,c", "d,e")


def test_names():
    from pdm.utils import esd as E
    assert E.checkpoint_name("Van Gogh", None, "xattn", 1, 1000) == "esd-vangogh_from_vangogh-xattn_1-epochs_1000"
    assert E.checkpoint_name("Van Gogh", "art", "noxattn", 1.0, 200) == "esd-vangogh_from_art-noxattn_1.0-epochs_200"
    assert (E.checkpoint_name("nudity, violence", None, "selfattn", 0.5, 3)
            == "esd-nudityviolence_from_nudityviolence-selfattn_0.5-epochs_3")
    assert E.checkpoint_path("models/", "Van Gogh", None, "xattn", 1, 1000) == "models//esd-vangogh_from_vangogh-xattn_1-epochs_1000.pt"


def test_draws_are_the_three_host_calls():
    from pdm.utils import esd as E
    np.random.seed(7)
    torch.manual_seed(7)
    gen = E.draws(2)
    got = [next(gen) for _ in range(20)]
    np.random.seed(7)
    torch.manual_seed(7)
    nsteps = 50
    for index, iteration, latents in got:
        assert index == np.random.choice(2, 1, replace=False)[0]
        assert iteration == torch.randint(1, nsteps - 1, (1,)).item()
        assert torch.equal(latents, torch.randn((1, 4, 64, 64)))
    assert {i for i, _, _ in got} == {0, 1} and all(1 <= it <= 48 for _, it, _ in got)


def test_timestep_index_through_the_scheduler():
    from pdm.pipelines.pruning_pipelines import DDIMScheduler
    from pdm.utils import esd as E
    sch = DDIMScheduler(prediction_type="v_prediction")
    for i in range(1, 49):
        assert E.timestep_index(i) == 20 * i
        assert E.prediction_timestep(sch, i) == 1000 - 20 * i
        assert len(sch.timesteps) == 50 and int(sch.timesteps[i]) == 981 - 20 * i        # where the sampled latent sits


def test_trainable_rule_on_the_tiny_topology():
    from pdm.utils import esd as E
    entries = _tiny_entries()
    names, kinds = E.entry_names(entries)
    assert len(names) == len(set(names))
    mods = {n.rsplit(".", 1)[0] for n, kd in zip(names, kinds) if kd in ("conv3", "lin")}
    linconv = [n for n in names if n.rsplit(".", 1)[0] in mods]
    x = E.trainable_names(names, kinds, "xattn")
    assert x and set(x) == {n for n in linconv if "attn2" in n}
    assert all(n.rsplit(".", 1)[0].split(".")[-1] in ("to_q", "to_k", "to_v", "0") for n in x)
    kv = [e for e in entries if e.key == "attn2_kv_all.weight"][0]
    assert {s[0] for s in kv.srcs} <= set(x) and kv in E.trainable_entries(entries, "xattn")
    nx = E.trainable_names(names, kinds, "noxattn")
    assert not set(x) & set(nx) and set(x) | set(nx) == set(linconv)
    s = E.trainable_names(names, kinds, "selfattn")
    assert s and set(s) == {n for n in linconv if "attn1" in n} and set(s) <= set(nx)
    for method in ("xattn", "noxattn", "selfattn"):
        chosen = E.trainable_names(names, kinds, method)
        assert not [n for n in chosen if "norm" in n], method
        assert [n for n in chosen if n.endswith(".bias")], method                  # a bias follows its Linear / Conv
    assert "time_emb_proj_all.weight" in {e.key for e in E.trainable_entries(entries, "noxattn")}
    assert "conv_in.weight" in nx and "conv_out.bias" in nx
    with pytest.raises(ValueError, match="empty parameter list"):
        E.trainable_names(names, kinds, "xattn-strict")
    for method in ("full", "nonsense"):
        with pytest.raises(NotImplementedError):
            E.trainable_names(names, kinds, method)
    with pytest.raises(NotImplementedError):
        E.check_train_method("full")


@pytest.mark.parametrize("method", ["xattn", "noxattn", "selfattn"])
def test_segments_cover_exactly_the_chosen_entries(method):
    from pdm.utils import esd as E
    entries = _tiny_entries()
    chosen = E.trainable_entries(entries, method)
    segs = E.segments(chosen)
    assert segs == sorted(segs)
    covered = set()
    end = -1
    for off, n in segs:
        assert off % 128 == 0 and n % 128 == 0 and n > 0
        assert off > end, "disjoint and not adjacent (neighbours are merged)"
        end = off + n
        covered.update(range(off // 128, (off + n) // 128))
    want = set()
    for e in chosen:
        want.update(range(e.off // 128, (e.off + e.numel + 127) // 128))
    assert covered == want
    other = set()
    for e in entries:
        if e not in chosen:
            other.update(range(e.off // 128, (e.off + e.numel + 127) // 128))
    assert not covered & other
    assert len(segs) < len(chosen)                                # a weight and its bias are neighbours at least once


def test_nest_round_trip():
    from pdm.utils import esd as E
    from pdm.utils.erasure_utils import esd_state_dict
    flat = {"down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k.weight": torch.randn(4, 3),
            "down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_out.0.weight": torch.randn(3, 4),
            "down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_out.0.bias": torch.randn(3),
            "up_blocks.1.resnets.0.conv_shortcut.weight": torch.randn(4, 2, 1, 1)}
    nested = E.nest_state_dict(flat)
    assert set(nested) == {"unet.down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k",
                           "unet.down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_out.0",
                           "unet.up_blocks.1.resnets.0.conv_shortcut"}
    assert set(nested["unet.down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k"]) == {"weight"}
    for back in (esd_state_dict(nested), E.unnest_state_dict(nested)):
        assert set(back) == set(flat) and all(torch.equal(back[n], flat[n]) for n in flat)
