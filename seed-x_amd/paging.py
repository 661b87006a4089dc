"""Page bookkeeping of the paged KV cache (``LlamaForCausalLM(kv_pages=N)``) — host logic only, no GPU and no torch.

The cache is ONE pool of ``n_pages`` pages of ``page_size`` key rows per layer, shared by every slot of the lock-step batch, and one
page table per slot (the same page index names the slot's rows in every layer's pool). ``PagePool`` decides which pages a slot holds;
``LlamaForCausalLM.kv_reserve`` / ``kv_release`` write its decisions into the device table the kernels read.

  * pages are numbered 1 .. n_pages. Page 0 is the NULL page: all zeros, never handed out, never written — every table entry without a
    reservation names it,
  * the free list is LIFO and the pool is deterministic: the same calls give the same pages (a freed page is the next one handed out,
    lowest index first on a fresh pool),
  * ``reserve(slot, n_rows)`` EXTENDS the slot's capacity to at least ``n_rows`` rows, so it is idempotent; it grants everything or
    nothing (False: the pool cannot cover it, and nothing changed),
  * ``release(slot)`` gives every page of the slot back.
"""

PAGE_SIZES = (32, 64, 128)        # powers of two and multiples of 32, the key tile of the MFMA prefill kernel: no tile straddles a page


def pages_for(n_rows, page_size):
    """Pages that hold ``n_rows`` key rows."""
    return (max(0, int(n_rows)) + int(page_size) - 1) // int(page_size)


class PagePool:
    def __init__(self, n_pages, page_size, n_slots, max_rows):
        """``max_rows``: the per-slot ceiling (``max_cache_len``): a slot's page list never grows past ceil(max_rows / page_size)."""
        if page_size not in PAGE_SIZES:
            raise ValueError(f"PagePool: page_size must be one of {PAGE_SIZES}, not {page_size!r}")
        if n_pages < 1 or n_slots < 1 or max_rows < 1:
            raise ValueError(f"PagePool: n_pages={n_pages}, n_slots={n_slots}, max_rows={max_rows} must all be >= 1")
        self.n_pages, self.page_size, self.n_slots, self.max_rows = int(n_pages), int(page_size), int(n_slots), int(max_rows)
        self.width = pages_for(self.max_rows, self.page_size)            # entries of a slot's table row
        self._free = list(range(self.n_pages, 0, -1))                    # a stack: pop() hands out 1, 2, ... on a fresh pool
        self._pages = [[] for _ in range(self.n_slots)]
        self.peak = 0                                                    # most pages ever held at once

    @property
    def free(self):
        """Pages nobody holds."""
        return len(self._free)

    @property
    def used(self):
        return self.n_pages - len(self._free)

    def pages(self, slot):
        """The slot's pages in row order: entry i holds its key rows [i * page_size, (i + 1) * page_size)."""
        return list(self._pages[slot])

    def capacity(self, slot):
        """Key rows the slot's pages hold."""
        return len(self._pages[slot]) * self.page_size

    def need(self, slot, n_rows):
        """Pages ``reserve(slot, n_rows)`` would take from the free list."""
        return max(0, pages_for(n_rows, self.page_size) - len(self._pages[slot]))

    def reserve(self, slot, n_rows):
        """Extends the slot's capacity to at least ``n_rows`` rows. True: done (possibly nothing to do); False: the free pages do not
        cover it, or ``n_rows`` exceeds the per-slot ceiling — nothing was granted."""
        if n_rows > self.max_rows:
            return False
        k = self.need(slot, n_rows)
        if k > len(self._free):
            return False
        for _ in range(k):
            self._pages[slot].append(self._free.pop())
        self.peak = max(self.peak, self.used)
        return True

    def release(self, slot):
        """Gives the slot's pages back (last page first onto the stack: the slot's first page is the next one handed out). Returns
        how many."""
        pages = self._pages[slot]
        self._pages[slot] = []
        self._free.extend(reversed(pages))
        return len(pages)

    def table_row(self, slot):
        """The slot's row of the device page table: its pages, then the null page."""
        pages = self._pages[slot]
        return pages + [0] * (self.width - len(pages))
