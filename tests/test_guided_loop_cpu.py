"""CPU: host logic of the one guided-sampling loop (FreeFinePipeline._guided_loop) for its three layouts -- which latent rows go to the UNet,
which of them are reference rows, how per-image CFG row maps merge, which recorded slot a step replays and where the reference tail is
dropped.  The expected lists are written out as the edit, removal and composition loops computed them one by one.  No kernel is launched."""
import torch

from freefine_amd.pipeline import BACKGROUND, COMPOSE, EDIT, FreeFinePipeline

EMPTY, CUP, DOG = (torch.full((77, 8), v) for v in (0.0, 1.0, 2.0))      # stand-ins for the embeddings of "", "a cup", "a dog"


def _pipe(**flags):
    p = FreeFinePipeline(None, None, None, None, None, device="cpu")
    for k, v in flags.items():
        setattr(p, k, v)
    return p


def _pair_text(prompt):
    """text rows of one edit / removal: negative prompt for both rows, then [prompt, ""]"""
    return torch.stack([EMPTY, EMPTY, prompt, EMPTY])


def _compose_text(R, prompts):
    return torch.stack([EMPTY] * (1 + R) + prompts + [EMPTY])


def test_pair_layouts_feed_the_deduplicated_rows():
    p = _pipe()
    for lay in (EDIT, BACKGROUND):
        # the reference stream runs against "" twice: 3 physical rows (edit_u, ref, edit_c)
        assert p._guided_rows(lay, [_pair_text(CUP)], 2) == ([0, 1, 2, 1], [0, 1, 0], [0, 1, 2], (False, True, False), [1])
        assert p._guided_rows(lay, [_pair_text(CUP), _pair_text(DOG)], 2) == ([0, 1, 2, 1], [0, 1, 0, 2, 3, 2], [0, 1, 2], (False, True, False), [1])
        # an empty edit prompt: the edit stream coincides too, 2 physical rows
        assert p._guided_rows(lay, [_pair_text(EMPTY)], 2) == ([0, 1, 0, 1], [0, 1], [0, 1], (False, True), [1])
        assert p._guided_rows(lay, [_pair_text(EMPTY)] * 2, 2) == ([0, 1, 0, 1], [0, 1, 2, 3], [0, 1], (False, True), [1])


def test_pair_layouts_fall_back_to_four_rows():
    four = (None, [0, 1, 0, 1], [0, 1, 2, 3], (False, True, False, True), [1, 3])
    for lay in (EDIT, BACKGROUND):
        # images disagree on which CFG rows coincide
        got = _pipe()._guided_rows(lay, [_pair_text(CUP), _pair_text(EMPTY), _pair_text(DOG)], 2)
        assert got == (None, [0, 1, 0, 1, 2, 3, 2, 3, 4, 5, 4, 5]) + four[2:]
        # de-duplication off
        assert _pipe(dedup_rows=False)._guided_rows(lay, [_pair_text(CUP)], 2) == four
        assert _pipe(dedup_rows=False)._guided_rows(lay, [_pair_text(CUP), _pair_text(DOG)], 2) == (None, [0, 1, 0, 1, 2, 3, 2, 3]) + four[2:]
    # no text coincides at all (a negative prompt): nothing to de-duplicate
    assert _pipe()._guided_rows(EDIT, [torch.stack([DOG, DOG, CUP, EMPTY])], 2) == four


def test_merged_row_map():
    p = _pipe()
    maps = [p._cfg_row_map(_pair_text(t), 2) for t in (CUP, DOG, EMPTY)]
    assert maps[0] == ([0, 1, 2, 1], [0, 1, 0], [0, 1, 2]) and maps[2] == ([0, 1, 0, 1], [0, 1], [0, 1])
    assert p._merge_row_maps(maps[:1]) == maps[0] and p._merge_row_maps(maps[:2]) == maps[0] and p._merge_row_maps([maps[2]] * 2) == maps[2]
    fallback = (None, [0, 1, 0, 1], [0, 1, 2, 3])
    assert p._merge_row_maps(maps) == fallback and p._merge_row_maps([maps[2], maps[0]]) == fallback
    off = _pipe(dedup_rows=False)._cfg_row_map(_pair_text(CUP), 2)
    assert off == (None, None, None) and p._merge_row_maps([off]) == fallback and p._merge_row_maps([off, off]) == fallback


def test_composition_layout_feeds_every_row_and_the_edit_row_twice():
    p = _pipe(dedup_rows=False)                               # no row map either way: the layout does not consult de-duplication
    for q in (p, _pipe()):
        assert q._guided_rows(COMPOSE, [_compose_text(1, [CUP])], 2) == (None, [0, 1, 0], [0, 1, 2, 3], (False, True, False), [1])
        assert q._guided_rows(COMPOSE, [_compose_text(1, [CUP])] * 2, 2) == (None, [0, 1, 0, 2, 3, 2], [0, 1, 2, 3], (False, True, False), [1])
        assert q._guided_rows(COMPOSE, [_compose_text(2, [CUP, DOG])], 3) == (None, [0, 1, 2, 0], [0, 1, 2, 3, 4, 5], (False, True, True, False), [1, 2])
        assert q._guided_rows(COMPOSE, [_compose_text(2, [CUP, DOG])] * 2, 3) == (None, [0, 1, 2, 0, 3, 4, 5, 3], [0, 1, 2, 3, 4, 5],
                                                                                  (False, True, True, False), [1, 2])


def test_replay_argument_slot_and_dropped_tail():
    """loop step j of n_act = num_steps - start_step replays slot n_act - j - 1; the reference tail is dropped on every scheduler step but the last"""
    num_steps, start_step = 10, 4
    n_act = num_steps - start_step
    slots = [[torch.full((1, 2), float(s)), torch.full((1, 3), 10.0 + s)] for s in range(n_act)]
    cache = dict(join=2, slots=slots)
    p = _pipe()
    assert p._reuse_arg(EDIT, None, (False, True, False), 4, num_steps, start_step) is None
    for j in range(n_act):
        i = start_step + j
        a = p._reuse_arg(EDIT, cache, (False, True, False), 4, num_steps, i)
        assert list(a) == ["mode", "join", "ref", "state", "drop_tail"] and (a["mode"], a["join"], a["ref"]) == ("replay", 2, (False, True, False))
        assert a["state"] is slots[n_act - j - 1]
        assert a["drop_tail"] is (i != num_steps - 1)
        # four physical rows: both reference rows are fed from the one recorded row
        b = p._reuse_arg(EDIT, cache, (False, True, False, True), 4, num_steps, i)
        assert b["ref"] == (False, True, False, True) and [s.shape[0] for s in b["state"]] == [2, 2]
        assert all(torch.equal(s, r.repeat_interleave(2, 0)) for s, r in zip(b["state"], slots[n_act - j - 1]))
        assert b["drop_tail"] is (i != num_steps - 1)
    assert [p._reuse_arg(EDIT, cache, (False, True, False), 4, num_steps, i)["drop_tail"] for i in range(start_step, num_steps)] == [True] * 5 + [False]
    assert not any(_pipe(drop_ref_tail=False)._reuse_arg(EDIT, cache, (False, True), 4, num_steps, i)["drop_tail"] for i in range(start_step, num_steps))


def test_stored_kv_argument():
    num_steps, start_step, R, P = 8, 3, 2, 3
    n_act = num_steps - start_step
    slots = [[(torch.full((R, 1), float(s)), torch.full((R, 1), -float(s)))] for s in range(n_act)]
    cache = dict(kv_from=10, slots=slots)
    for j in range(n_act):
        a = _pipe()._reuse_arg(COMPOSE, cache, (False, True, True, False), 1 + R + P, num_steps, start_step + j)
        assert a == dict(mode="replay_kv", kv_from=10, ref=(False, True, True, False), kv=slots[n_act - j - 1], text_sel=[0, 3, 4, 5])
        assert a["kv"] is slots[n_act - j - 1]
    a = _pipe()._reuse_arg(COMPOSE, cache, (False, True, False), 1 + 1 + 2, num_steps, start_step)
    assert a["text_sel"] == [0, 2, 3] and a["kv"] is slots[n_act - 1]
