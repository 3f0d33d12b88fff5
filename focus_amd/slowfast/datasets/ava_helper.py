"""The part of slowfast/datasets/ava_helper.py the AVA meter needs: the frame lists, which number the videos."""
import os
from collections import defaultdict


def load_image_lists(cfg, is_train):
    """ava_helper.py:16-66 -> (image_paths, video_idx_to_name).  Every row of the frame-list files of
    cfg.AVA.TRAIN_LISTS / TEST_LISTS (under cfg.AVA.FRAME_LIST_DIR; the first line is a header) reads
    'original_video_id video_id frame_id path labels'; a video's index is the order of its first appearance, and
    image_paths[index] lists its frames under cfg.AVA.FRAME_DIR."""
    image_paths = defaultdict(list)
    video_name_to_idx = {}
    video_idx_to_name = []
    for filename in (cfg.AVA.TRAIN_LISTS if is_train else cfg.AVA.TEST_LISTS):
        with open(os.path.join(cfg.AVA.FRAME_LIST_DIR, filename), "r") as f:
            f.readline()
            for line in f:
                row = line.split()
                assert len(row) == 5, "a frame-list row has 5 fields: %r" % (line,)
                if row[0] not in video_name_to_idx:
                    video_name_to_idx[row[0]] = len(video_idx_to_name)
                    video_idx_to_name.append(row[0])
                image_paths[video_name_to_idx[row[0]]].append(os.path.join(cfg.AVA.FRAME_DIR, row[3]))
    return [image_paths[i] for i in range(len(image_paths))], video_idx_to_name
