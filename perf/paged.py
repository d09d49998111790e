"""What the --paged option of the attention and decode drivers shares: contiguous caches scattered into page pools whose pages are
handed out in a seeded random order (never ascending), DESIGN.md §17."""
import torch


def random_table(B, max_pages, num_pages, seed, device):
    """int32 [B, max_pages]: B * max_pages distinct pages of a pool of num_pages, in a seeded random order"""
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(seed))
    return perm[:B * max_pages].view(B, max_pages).to(torch.int32).to(device)


def scatter(cache, table, page_size, num_pages):
    """the pool [num_pages, nkv, page_size, hd] that holds the contiguous cache [B, nkv, L, hd] behind `table`"""
    B, nkv, L, hd = cache.shape
    raw = torch.uint8 if cache.element_size() == 1 else torch.int16
    pool = torch.zeros(num_pages, nkv, page_size, hd, dtype=raw, device=cache.device)
    pool[table.long()] = cache.view(raw).view(B, nkv, L // page_size, page_size, hd).transpose(1, 2)
    return pool.view(cache.dtype)

