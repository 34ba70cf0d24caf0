"""TEST HELPER (not a test): a miniature of the reference's learning_phase_data tree -- the golden JPEGs of tests/golden/jpeg copied
under COCO file names, and sample JSONs in the layout gpv1_amd.datasets reads -- plus the task_configs / learning_datasets trees that
point at it."""
import json
import os
import shutil

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg')
# image_id -> golden file; c420_big is 120 x 160, gray_q80 a grey file (45 x 61), c422_odd_q60 29 x 43
IMAGES = {1: 'c420_big', 2: 'gray_q80', 3: 'c422_odd_q60', 4: 'c444_q90', 5: 'c420_opt_q30', 6: 'c420_rst_q80'}
SIZES = {1: (120, 160), 2: (45, 61), 3: (29, 43), 4: (48, 64), 5: (64, 80), 6: (50, 70)}
TASKS = {'cap': ('CocoCaptioning', 'coco_captioning', 'coco_cap'), 'det': ('CocoDetection', 'coco_detection', 'coco_det'),
         'cls': ('CocoClassification', 'coco_classification', 'coco_cls'), 'vqa': ('CocoVqa', 'coco_vqa', 'coco_vqa'),
         'refcocop': ('RefCocop', 'refcocop', 'refcocop')}


def _image(subset, image_id):
    H, W = SIZES[image_id]
    return {'subset': subset, 'image_id': image_id, 'H': H, 'W': W}


def samples_for(kind, subset, ids):
    """len(ids) samples of one task on the images `ids` of `subset`"""
    out = []
    for n, i in enumerate(ids):
        H, W = SIZES[i]
        s = {'image': _image(subset, i)}
        if kind == 'cap':
            s.update(query='describe the image', answer=f'w{n} w{n + 1} w{n + 2}', cap_id=100 + n)
        elif kind == 'vqa':
            s.update(query='what color is the cat', answer='w3', all_answers={'w1': 5, 'w2': 3, 'w3': 2}, question_id=200 + n)
        elif kind == 'det':
            s.update(query='locate the dog', boxes=[[0.1 * W, 0.2 * H, 0.3 * W, 0.4 * H], [0.5 * W, 0.5 * H, 0.25 * W, 0.25 * H]][:1 + n % 2],
                     id=300 + n, category_name='dog')
        elif kind == 'cls':
            s.update(query='what is this object', answer=f'w{4 + n}', boxes=[10.7, 100.2, 3, 40] if i == 1 else [0.25 * W, 0.25 * H, 0.5 * W, 0.5 * H],
                     id=400 + n)
        else:
            s.update(query='the red umbrella', boxes=[[0.2 * W, 0.1 * H, 0.4 * W, 0.5 * H]], sent_id=500 + n)
        out.append(s)
    return out


def make_tree(root, plan, image_size=(96, 128)):
    """plan: {kind: {subset: [image ids]}} -> task_configs dict (plain, no interpolation) for gpv1_amd.datasets.
    Images land in root/images/<subset>2014/, samples in root/<task_config>/<subset>.json."""
    root = str(root)
    image_dir = os.path.join(root, 'images')
    tc = {'image_dir': image_dir, 'image_size': {'H': image_size[0], 'W': image_size[1]}, 'read_image': True}
    for kind, subsets in plan.items():
        _, cfg_name, _ = TASKS[kind]
        os.makedirs(os.path.join(root, cfg_name), exist_ok=True)
        tc[cfg_name] = {'image_dir': image_dir, 'image_size': dict(tc['image_size']), 'read_image': True, 'samples': {}, 'max_samples': {}}
        for subset, ids in subsets.items():
            img_subset = subset + '2014'
            os.makedirs(os.path.join(image_dir, img_subset), exist_ok=True)
            for i in ids:
                dst = os.path.join(image_dir, img_subset, f'COCO_{img_subset}_{i:012d}.jpg')
                if not os.path.exists(dst):
                    shutil.copyfile(os.path.join(GOLD, IMAGES[i] + '.jpg'), dst)
            path = os.path.join(root, cfg_name, subset + '.json')
            with open(path, 'w') as f:
                json.dump(samples_for(kind, img_subset, ids), f)
            tc[cfg_name]['samples'][subset] = path
            tc[cfg_name]['max_samples'][subset] = None
    return tc


def learning_datasets(kinds):
    return {TASKS[k][0]: {'task_config': TASKS[k][1], 'name': TASKS[k][2]} for k in kinds}
