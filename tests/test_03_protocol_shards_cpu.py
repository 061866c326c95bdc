"""Method one, method two and supervised fine-tuning from a protocol root of shards, the part that needs no GPU: the root
(`shards.protocol_splits`), class indices made from the joint label ids (`shards.class_index_table` / `class_indices`,
`protocols.ProtocolRoot`) against `label_batch_to_species_idx` on the same samples' label dictionaries, and the three scripts' argument
checks, all of which run before any GPU work."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd"))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
TINY = os.path.join(ROOT, "tests", "golden", "tiny_shard")
LEVELS = ("order", "family", "genus", "species")
CONFIG = ["model_config=lora_vit_lora_barcode_bert_ssl", "model_config.load_ckpt=false"]


def _write(path, species, first=0):
    """A shard of len(species) samples of the tiny golden shard; genus = the species' first word, one family, one order."""
    from bioscanclip.util import shards
    tiny = shards.Shard(TINY)
    pick = [(first + i) % len(tiny) for i in range(len(species))]
    taxonomy = {"order": ["Diptera"] * len(species), "family": ["Fam"] * len(species), "genus": [s.split(" ")[0] for s in species],
                "species": list(species)}
    shards.write_shard(str(path), [tiny.image(i) for i in pick], [tiny.barcode(i) for i in pick], np.array(tiny.input_ids)[pick],
                       np.array(tiny.token_type_ids)[pick], np.array(tiny.attention_mask)[pick], [f"S{i:03d}" for i in pick],
                       taxonomy=taxonomy, split=os.path.basename(str(path)))
    return str(path)


TRAIN = ["A a", "B b", "A a", "C c", "B b", "A d", "C c"]                # first appearance: A a, B b, C c, A d
VAL = ["C c", "A a", "Z z", "A d", "B b", "Z z", "A a"]                  # "Z z" is no class


def _root(tmp_path):
    from bioscanclip.util import shards
    for k, name in enumerate(shards.PROTOCOL_SPLITS):
        _write(tmp_path / name, TRAIN if name == "train_seen" else VAL, first=k)
    return str(tmp_path)


def test_protocol_splits_names_the_reference_splits(tmp_path):
    from bioscanclip.util import shards
    root = _root(tmp_path)
    (tmp_path / "notes").mkdir()                                         # other sub-directories are ignored
    at = lambda name: os.path.join(root, name)
    assert shards.PROTOCOL_SPLITS == ("train_seen", "seen_keys", "val_unseen_keys", "test_unseen_keys", "val_seen", "val_unseen",
                                      "test_seen", "test_unseen")
    assert shards.protocol_splits(root) == tuple(at(n) for n in shards.PROTOCOL_SPLITS)
    assert shards.protocol_splits(root, ("val_seen", "train_seen")) == (at("val_seen"), at("train_seen"))
    with pytest.raises(ValueError, match="all_keys"):
        shards.protocol_splits(root, ("train_seen", "all_keys"))         # not a split of the protocols
    os.remove(at(os.path.join("test_unseen", "meta.json")))              # the directory is there but is no shard any more
    with pytest.raises(ValueError) as exc:
        shards.protocol_splits(root)
    assert "'test_unseen'" in str(exc.value) and root in str(exc.value) and "train_seen, seen_keys" in str(exc.value)
    assert shards.protocol_splits(root, ("train_seen", "val_seen")) == (at("train_seen"), at("val_seen"))   # these do not need it
    import shutil
    shutil.rmtree(at("val_unseen"))
    with pytest.raises(ValueError, match="'val_unseen'"):
        shards.protocol_splits(root)                                     # an absent split
    with pytest.raises(ValueError, match="'train_seen'"):
        shards.protocol_splits(at("notes"), ("train_seen",))            # a plain directory


CLASS_LISTS = {
    "first_appearance": ["A a", "B b", "C c", "A d"],
    "permuted": ["C c", "A d", "A a", "B b"],
    "duplicate": ["B b", "A a", "B b", "C c", "A a", "A d"],            # list.index takes the first
}


@pytest.mark.parametrize("case", sorted(CLASS_LISTS))
def test_class_indices_equal_list_index_on_the_label_dictionaries(tmp_path, case):
    from bioscanclip.epoch.fine_tuning_epoch import label_batch_to_species_idx
    from bioscanclip.hip.protocols import ProtocolRoot
    from bioscanclip.util import shards
    root = _root(tmp_path)
    classes = CLASS_LISTS[case]
    proto = ProtocolRoot(root, ("val_seen", "train_seen"), device="cpu")
    assert proto.names == ("train_seen", "val_seen")                      # encoded with the training split first, whatever was asked
    assert proto.vocab["species"] == ["A a", "B b", "C c", "A d", "Z z"]
    assert proto.first_appearance_classes("train_seen") == CLASS_LISTS["first_appearance"]
    train_col, val_col = proto.class_columns(classes, "train_seen", "val_seen")
    assert train_col.dtype == np.int32 and train_col.shape == (len(TRAIN),)
    sh = shards.Shard(os.path.join(root, "train_seen"))
    dicts = sh.label_dicts(range(len(sh)))
    batch = {lv: [d[lv] for d in dicts] for lv in LEVELS}
    assert train_col.tolist() == label_batch_to_species_idx(batch, classes).tolist()
    in_list = [i for i, s in enumerate(VAL) if s in classes]
    assert val_col[in_list].tolist() == [classes.index(VAL[i]) for i in in_list]
    outside = [i for i, s in enumerate(VAL) if s not in classes]
    assert outside == [2, 5] and val_col[outside].tolist() == [shards.NOT_A_CLASS] * 2 and shards.NOT_A_CLASS == -1
    table = shards.class_index_table(proto.vocab["species"], classes)
    assert table.dtype == np.int32 and np.array_equal(shards.class_indices(proto.ids["val_seen"], table), val_col)
    assert np.array_equal(shards.class_indices(proto.ids["val_seen"][:, 3], table), val_col)


def test_sorted_class_list_equals_the_label_map_of_a_walk(tmp_path):
    """``ProtocolRoot.sorted_class_list`` against ``load_all_seen_species_name_and_create_label_map`` fed the same label dictionaries
    in storage order, and the member table against the names."""
    import method_two_fine_tuning_and_eval as M
    from bioscanclip.hip.protocols import LabelRows, ProtocolRoot
    from bioscanclip.util import shards
    root = _root(tmp_path)
    proto = ProtocolRoot(root, shards.PROTOCOL_SPLITS, device="cpu")
    sh = proto.shards["train_seen"]
    batches = []
    for i in range(0, len(sh), 3):
        dicts = sh.label_dicts(range(i, min(i + 3, len(sh))))
        batches.append((None,) * 6 + ({lv: [d[lv] for d in dicts] for lv in LEVELS},))
    ref_map, ref_rows = M.load_all_seen_species_name_and_create_label_map(batches)
    label_map, rows, class_table = proto.sorted_class_list("train_seen")
    assert label_map == ref_map and list(label_map) == list(ref_map) == sorted(ref_map) and rows == ref_rows
    assert class_table.dtype == np.int32 and class_table.shape == (4, 4)
    assert [LabelRows(class_table, proto.vocab)[c] for c in range(4)] == [ref_rows[c] for c in range(4)]
    member = proto.member_table("train_seen")
    assert member.dtype == np.int32 and member.tolist() == [1, 1, 1, 1, 0]
    assert sorted(proto.species_names("val_seen", "val_unseen")) == sorted(set(VAL))
    assert proto.member_table("val_seen").tolist() == [1, 1, 1, 1, 1]


def test_script_argument_validation(tmp_path):
    import method_one_eval
    import method_two_fine_tuning_and_eval
    import supervised_fine_tune
    root = _root(tmp_path / "root")
    for script, first_split in ((method_one_eval, "seen_keys"), (method_two_fine_tuning_and_eval, "train_seen")):
        with pytest.raises(ValueError, match="synthetic_eval_batches.*eval_shards"):
            script.main(CONFIG + [f"eval_shards={root}", "synthetic_eval_batches=1"])
        with pytest.raises(ValueError, match="hip_jpeg_entropy"):
            script.main(CONFIG + [f"eval_shards={root}", "hip_jpeg_entropy=cpu"])
        with pytest.raises(ValueError, match=f"'{first_split}'"):
            script.main(CONFIG + [f"eval_shards={tmp_path}"])           # a directory, but no protocol root
    with pytest.raises(ValueError, match="synthetic_steps_per_epoch"):
        method_two_fine_tuning_and_eval.main(CONFIG + [f"eval_shards={root}", "synthetic_steps_per_epoch=2"])
    with pytest.raises(NotImplementedError, match="dataset=synthetic"):
        supervised_fine_tune.main(CONFIG + ["dataset=insect"])            # any other string keeps raising
    with pytest.raises(ValueError, match="'train_seen'"):
        supervised_fine_tune.main(CONFIG + [f"dataset={tmp_path}"])       # a directory, but not a root
    with pytest.raises(ValueError, match="hip_jpeg_entropy"):
        supervised_fine_tune.main(CONFIG + [f"dataset={root}", "hip_jpeg_entropy=cpu"])


def test_loader_label_mode_is_validated_before_any_gpu_work(tmp_path):
    from bioscanclip.util import shards
    assert shards.LABEL_MODES == (None, "ids")
    with pytest.raises(ValueError, match="labels"):
        shards.ShardLoader(_write(tmp_path / "s", VAL), 4, for_training=False, labels="names", device="cpu")
