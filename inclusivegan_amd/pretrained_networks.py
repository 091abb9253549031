"""Loading of network snapshots for the inference scripts (reference: pretrained_networks.py:57-78).

`load_networks(path)` opens a snapshot pickle -- this engine's or the reference's layout -- and returns its live networks,
cached per path like the reference's.  The reference also maps 'gdrive:networks/...' names to URLs and downloads them; this
package contains no code that opens a connection, so a URL or a gdrive name raises and asks for a local file."""
from .training import misc

_cached_networks = dict()


def _is_remote(path_or_gdrive_path):
    s = str(path_or_gdrive_path)
    return s.startswith('gdrive:') or '://' in s


def get_path_or_url(path_or_gdrive_path):
    """The identity for local paths (pretrained_networks.py:57-58 looks gdrive names up in its URL table)."""
    if _is_remote(path_or_gdrive_path):
        raise RuntimeError('%r is not a local file: this package does not download. Fetch the pickle by other means and pass its path.'
                           % (path_or_gdrive_path,))
    return path_or_gdrive_path


def load_networks(path_or_gdrive_path, device=None):
    """The snapshot's objects, typically (G, D, Gs), as live Networks (pretrained_networks.py:64-78)."""
    path = get_path_or_url(path_or_gdrive_path)
    key = (path, str(device))
    if key not in _cached_networks:
        _cached_networks[key] = misc.as_networks(misc.load_pkl(path), device=device)
    return _cached_networks[key]
