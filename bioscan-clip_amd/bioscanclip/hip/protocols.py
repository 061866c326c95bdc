"""The seen / unseen protocols (method one, method two) and supervised fine-tuning fed from a protocol root of shards.

A protocol root (``shards.protocol_splits``) holds the reference's splits as shard directories.  ``ProtocolRoot`` encodes the labels
of the splits it is asked for together (``shards.taxonomy_ids``, the training split first, so species ids follow the class list's order
of first appearance), and everything label-shaped downstream is an int32 array made from those ids with numpy: class-index columns
(``class_columns``), the class table of method two (``sorted_class_list``), member tables (``member_table``).  No label dictionary is
built per sample and no Python loop runs over samples.

    proto = ProtocolRoot(root, ("seen_keys", "val_unseen_keys", "test_unseen_keys", "val_seen", "val_unseen"))
    keys = method_one_keys(proto, model, device)                            # both key indices, built once as the batches arrive
    seen, unseen = (method_one_split(proto, name, model, device, keys) for name in ("val_seen", "val_unseen"))

Each split is walked once (``features.extract_split`` with only the towers it needs: image for queries and seen keys, DNA for the
unseen keys); features, indices, confidences and label ids stay on the GPU.
"""
import numpy as np

from ..util import shards
from .features import extract_split
from .method_one import MethodOneSplit
from .method_two import MethodTwoSplit
from .retrieval import LEVELS, Labels, RetrievalIndex, decode_labels

SPECIES = LEVELS.index("species")
UNSEEN_KEY_SPLITS = ("val_unseen_keys", "test_unseen_keys")


class LabelRows:
    """The label dictionaries of an id array, made one at a time when somebody indexes them (``merged_predictions`` does, for the
    keys a query hit): stands in for the list of dictionaries of a key set without building it."""

    def __init__(self, ids, vocab):
        self.ids, self.vocab = ids, vocab

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, i):
        return {lv: self.vocab[lv][int(c)] for lv, c in zip(LEVELS, self.ids[i])}


class ProtocolRoot:
    """The splits ``names`` of a protocol root with their labels encoded together: ``ids[name]`` int32 ``[n, 4]`` and one ``vocab``.
    The splits are encoded in the order of ``shards.PROTOCOL_SPLITS`` (``train_seen``, else ``seen_keys``, first)."""

    def __init__(self, root, names, batch_size=40, entropy="host", device="cuda"):
        shards.protocol_splits(root, names)                        # refuses an unknown name, an absent split, a plain directory
        self.names = tuple(n for n in shards.PROTOCOL_SPLITS if n in tuple(names))
        paths = shards.protocol_splits(root, self.names)
        self.root, self.batch_size, self.entropy, self.device = str(root), int(batch_size), entropy, device
        self.shards = {n: shards.Shard(p) for n, p in zip(self.names, paths)}
        arrays, self.vocab = shards.taxonomy_ids([self.shards[n] for n in self.names], LEVELS)
        self.ids = dict(zip(self.names, arrays))

    def loader(self, name, labels="ids", batch_size=None, shuffle=False, for_training=False, seed=0):
        """The split's ``ShardLoader`` without text: evaluation transform and order unless told otherwise; ``labels="ids"`` (default)
        yields sample indices in slot 6, ``labels=None`` the label dictionaries the host functions read."""
        return shards.ShardLoader(self.shards[name], self.batch_size if batch_size is None else int(batch_size), shuffle=shuffle, seed=seed,
                                  for_training=for_training, with_text=False, device=self.device, entropy=self.entropy, labels=labels)

    def labels_of(self, name):
        return self.ids[name], self.vocab

    def species_ids(self, *names):
        """The distinct species ids of the named splits."""
        return np.unique(np.concatenate([self.ids[n][:, SPECIES] for n in names]))

    def species_names(self, *names):
        return [self.vocab["species"][i] for i in self.species_ids(*names).tolist()]

    def member_table(self, *names):
        """int32 0/1 over the species ids: 1 for the species of the named splits (``method_one.member_share``'s table)."""
        table = np.zeros(len(self.vocab["species"]), dtype=np.int32)
        table[self.species_ids(*names)] = 1
        return table

    def first_appearance_classes(self, name="train_seen"):
        """The class list of ``supervised_fine_tune.unique_species`` over the unshuffled split: its species in order of first
        appearance."""
        from .retrieval import first_appearance_order
        return [self.vocab["species"][i] for i in first_appearance_order(self.ids[name][:, SPECIES]).tolist()]

    def sorted_class_list(self, name="train_seen"):
        """``load_all_seen_species_name_and_create_label_map`` of the split without walking it: ``(label_to_index_dict,
        idx_to_all_labels, class_table)`` -- the sorted species numbered from 0, per class the species with the order / family / genus
        of its first appearance, and the same rows as int32 ``[C, 4]`` ids."""
        ids = self.ids[name]
        uniq, first = np.unique(ids[:, SPECIES], return_index=True)
        rows = {self.vocab["species"][s]: ids[r] for s, r in zip(uniq.tolist(), first.tolist())}
        classes = sorted(rows)
        class_table = np.ascontiguousarray(np.stack([rows[s] for s in classes]), dtype=np.int32)
        label_to_index = {s: c for c, s in enumerate(classes)}
        idx_to_all_labels = {c: {'species': s, **{lv: self.vocab[lv][int(rows[s][j])] for j, lv in enumerate(LEVELS) if lv != 'species'}}
                             for c, s in enumerate(classes)}
        return label_to_index, idx_to_all_labels, class_table

    def class_columns(self, classes, *names):
        """Per named split the int32 ``[n]`` class-index column for the class list ``classes`` (``shards.NOT_A_CLASS`` where a
        species is not listed): one look-up table over the species ids, made once on the host."""
        table = shards.class_index_table(self.vocab["species"], classes)
        return [shards.class_indices(self.ids[n], table, SPECIES) for n in names]

    def targets(self, classes, name):
        """The ``targets_of`` hook of the fine-tuning drivers for the named split's ``loader(name, labels="ids")``."""
        from ..epoch.fine_tuning_epoch import ResidentTargets
        return ResidentTargets(self.class_columns(classes, name)[0], self.device)


def unseen_key_index(proto, model, device, width=768):
    """(RetrievalIndex over the DNA features of val + test unseen keys, their ``Labels``): one index for both splits, filled batch by
    batch while each is walked once with the DNA tower alone.  ``width``: the towers' output width (an index of another width
    refuses the rows)."""
    counts = [len(proto.shards[n]) for n in UNSEEN_KEY_SPLITS]
    index, row0 = RetrievalIndex.empty(sum(counts), int(width), device), 0
    for name, n in zip(UNSEEN_KEY_SPLITS, counts):
        extract_split(proto.loader(name), model, device, labels=proto.labels_of(name), towers=("dna",),
                      append_to={"encoded_dna_feature": (index, row0)})
        row0 += n
    ids = np.concatenate([proto.ids[n] for n in UNSEEN_KEY_SPLITS])
    return index, Labels(ids, device)


def method_one_keys(proto, model, device, width=768):
    """``(seen_index, seen_labels, unseen_index, unseen_labels)``: the image features of ``seen_keys`` and the DNA features of the
    unseen key splits as search indices, each key split walked once."""
    seen = extract_split(proto.loader("seen_keys"), model, device, for_key_set=True, index=True, labels=proto.labels_of("seen_keys"),
                         towers=("image",))
    unseen_index, unseen_labels = unseen_key_index(proto, model, device, width)
    return seen.indices["encoded_image_feature"], Labels(seen.label_ids, device), unseen_index, unseen_labels


def method_one_split(proto, name, model, device, keys):
    """The ``MethodOneSplit`` of one query split: one walk with the image tower, then the two searches on resident tables."""
    seen_index, seen_labels, unseen_index, unseen_labels = keys
    q = extract_split(proto.loader(name), model, device, labels=proto.labels_of(name), towers=("image",))
    return MethodOneSplit.from_queries(seen_index, seen_labels, unseen_index, unseen_labels, q.tables["encoded_image_feature"], q.label_ids,
                                       max_k=5, levels=LEVELS)


def method_two_split(proto, name, classifier, n_classes, class_table, original_model, device, unseen_index, unseen_labels, top_k=5):
    """The ``MethodTwoSplit`` of one query split: one walk in which the fine-tuned classifier's softmax top-k goes straight into the
    split's ``[Q, top_k]`` tables and the original model's image features into the feature table."""
    q = extract_split(proto.loader(name), original_model, device, labels=proto.labels_of(name), towers=("image",), classifier=classifier,
                      n_classes=n_classes, top_k=top_k)
    return MethodTwoSplit.from_classifier(q.confidences, q.class_indices, class_table, unseen_index, unseen_labels,
                                          q.tables["encoded_image_feature"], q.label_ids, levels=LEVELS)


def ground_truth(proto, name):
    """The split's label dictionaries in sample order (the ``gt_labels`` entry of the protocols' output dictionaries)."""
    return decode_labels(proto.ids[name], proto.vocab, LEVELS)
